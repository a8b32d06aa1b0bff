// stackrl_hip.hip — C-ABI of libstackrl_hip.so (include/stackrl_hip.h): host side.  Built by stackrl_amd/build.py.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <stddef.h>

#include <memory>
#include "../../include/stackrl_hip.h"
#include "settle.hip"
#include "render.hip"
#include "view.hip"
#include "camera.hip"
#include "state.hip"
#include "contacts.hip"
#include "push.hip"
#include "env_host.h"   // fail / g_err, derive, layout, step_variant_of, state_layout, MeshTable: no HIP calls

namespace {

#define HIP_TRY(expr)                                                                                                  \
  do {                                                                                                                 \
    const hipError_t _e = (expr);                                                                                      \
    if (_e != hipSuccess) { snprintf(g_err, sizeof g_err, "%s: %s", #expr, hipGetErrorString(_e)); return SRL_EHIP; }  \
  } while (0)

#define SRL_TRY(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)   // (a code of ours: the text is set)

struct EventPair { hipEvent_t a, b; int which; };

// device memory freed with its owner; move-only (the move constructor deletes the copies); alloc(count) is for an empty buffer
template <class T> class DevBuf {
  T* p = nullptr;
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.release()) {}
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t count) { return hipMalloc((void**)&p, sizeof(T) * count); }
  T* get() const { return p; }
  T* release() { T* q = p; p = nullptr; return q; }
  void swap(DevBuf& o) { T* q = p; p = o.p; o.p = q; }
};

}  // namespace

struct srl_env {
  DevParams P;                                                         // raw copies of the pointers the kernels read; owned below
  DevBuf<EnvHdr> hdr; DevBuf<float> blob, H; DevBuf<int32_t> flags;    // P.hdr, P.blob, P.H, P.flags
  DevBuf<MeshHdr> d_mh; DevBuf<float4> d_mv, d_mp; DevBuf<uchar4> d_mt, d_me;   // the mesh table (srl_load_meshes): P.mh ...
  DevBuf<float> d_objmap; DevBuf<uint8_t> d_objmap_u8;
  DevBuf<DevParams> d_P;      // device copy of P for the settle kernel (re-uploaded whenever P changes)
  bool P_dirty = true;
  DevBuf<uint2> d_codec;      // overhead depth codec tabulated over the lattice of fl(FAR - z) (DevParams::codec)
  // where srl_reset sends the reward / done of a reset (zeros nobody reads, utils.py:545-552): owned by the handle and
  // allocated in srl_create, so that srl_reset allocates nothing and handles share no buffer
  DevBuf<float> d_reset_r; DevBuf<uint8_t> d_reset_d;
  StepVariant step_variant = STEP_4W_PP1;   // chosen by srl_load_meshes
  int concurrent_envs = 0;   // srl_set_concurrent_envs: envs stepping on the device at the same time, over all handles
  // launch order of srl_k_step (settle.hip, srl_k_order_*): -1 = by batch size (on when the envs outnumber the resident
  // workgroups), 0 = index order, 1 = highest release first (srl_set_launch_order)
  int order_mode = -1;
  DevBuf<unsigned long long> d_order_keys; DevBuf<int32_t> d_order;
  // staged rock records (render.hip, srl_k_stage -> srl_k_render): [n_envs][episode_length][SRL_STAGE_STRIDE] float4;
  // the explicit-pose hook (srl_render_heightmap) has its own, SRL_MAX_BODIES slots per env, allocated at its first use
  DevBuf<float4> d_stage, d_stage_ext;
  // the records are made by the settle kernel's tail for the envs it steps; after a test hook has moved bodies behind its
  // back (srl_set_body_state, srl_step_simulation) the next render is preceded by srl_k_stage over the whole batch
  bool stage_dirty = false;
  uint64_t mesh_hash = 0;     // of the arrays srl_load_meshes was given: part of the state signature (srl_state_signature)
  size_t step_lds = 0, render_lds = 0;
  bool profiling = false;
  std::vector<EventPair> pending;
  std::vector<hipEvent_t> pool;
  // 0 settle, 1 render, 2 srl_k_stage (hook / stale records only), 3 the two launch-order kernels, 4 srl_k_contact_points and the
  // three kernels of push.hip (kept out of the step's three; no export reports it)
  float acc_ms[5] = {0, 0, 0, 0, 0};
  int acc_n[5] = {0, 0, 0, 0, 0};
};

namespace {

static_assert(HOST_M_WORDS == M_WORDS && HOST_CG_WORDS == SRL_CG_WORDS, "env_host.h restates settle.hip's M_WORDS and solver.h's SRL_CG_WORDS");

// the kernel of each row of k_step_variants (env_host.h)
decltype(&srl_k_step) const k_step_kernels[STEP_VARIANTS] = {srl_k_step, srl_k_step_pp1, srl_k_step_pp2, srl_k_step_t128};

hipEvent_t get_event(srl_env* env) {
  if (!env->pool.empty()) { hipEvent_t e = env->pool.back(); env->pool.pop_back(); return e; }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// Per-kernel timing (bench.py's roofline leg): the two events are attached to the dispatch itself (hipExtLaunchKernelGGL),
// so they carry the kernel's own begin / end timestamps on its stream — what rocprofv3 reports for the dispatch — and not
// the two marker packets of hipEventRecord calls around it (about 3 us on a 44 us kernel).
EventPair prof_pair(srl_env* env, int which) {
  EventPair p; p.a = nullptr; p.b = nullptr; p.which = which;
  if (env->profiling) { p.a = get_event(env); p.b = get_event(env); env->pending.push_back(p); }
  return p;
}
#define SRL_LAUNCH(env_, which_, kernel_, grid_, block_, lds_, st_, ...)                                           \
  do {                                                                                                             \
    const EventPair ev_ = prof_pair(env_, which_);                                                                 \
    if (ev_.a) hipExtLaunchKernelGGL(kernel_, grid_, block_, lds_, st_, ev_.a, ev_.b, 0, __VA_ARGS__);             \
    else hipLaunchKernelGGL(kernel_, grid_, block_, lds_, st_, __VA_ARGS__);                                       \
  } while (0)

// Ordered launch (settle.hip, srl_k_order_*): worth its two small kernels only when a launch takes several rounds of
// resident workgroups — 2,048 envs or more on this 256-CU part (at most four env workgroups per CU) — and possible while the
// batch's keys fit the sort's LDS (16,384 envs = 128 KB).
constexpr int SRL_ORDER_MIN_ENVS = 2048, SRL_ORDER_MAX_ENVS = 16384;
bool launch_ordered(const srl_env* env) {
  const int n = env->P.c.n_envs;
  if (n > SRL_ORDER_MAX_ENVS || n < 2 || !env->d_order.get()) return false;
  return env->order_mode == 1 || (env->order_mode < 0 && n >= SRL_ORDER_MIN_ENVS);
}

// the render kernel of each observation element type, indexed by SRL_DTYPE_* (render.hip SRL_RENDER_KERNEL)
typedef void (*render_kernel_t)(DevParams, const float4*, int, uint8_t*, uint8_t*, float*, uint8_t*, const int32_t*, float*);
const render_kernel_t k_render_of_dtype[SRL_DTYPE_FLOAT64 + 1] = {srl_k_render, srl_k_render_u16, srl_k_render_u32, srl_k_render_u64,
                                                                  srl_k_render_f16, srl_k_render_f32, srl_k_render_f64};

int launch_step_render(srl_env* env, const int64_t* action, void* obs_map, void* obs_obj, float* reward, uint8_t* done,
                       hipStream_t st, int force_reset) {
  if (!env->d_mh.get()) return fail(SRL_ENOMESH, "srl_load_meshes must be called first");
  const DevParams& P = env->P;
  const int n = P.c.n_envs;
  if (env->P_dirty) {   // only after create / load_meshes / seed (all of which leave the device idle), never in steady state:
    // a blocking copy, so that the kernels below read the parameters whatever stream they run on
    HIP_TRY(hipMemcpy(env->d_P.get(), &env->P, sizeof(DevParams), hipMemcpyHostToDevice));
    env->P_dirty = false;
  }
  const DevParams* dP = env->d_P.get();
  const int32_t* order = nullptr;
  if (force_reset == 0 && launch_ordered(env)) {   // a placement call of a batch that outnumbers the resident workgroups
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    SRL_LAUNCH(env, 3, srl_k_order_keys, dim3(n), dim3(64), 0, st, dP, action, env->d_order_keys.get());
    SRL_LAUNCH(env, 3, srl_k_order_sort, dim3(1), dim3(1024), (size_t)np2 * 8, st, (const unsigned long long*)env->d_order_keys.get(), n, np2,
               env->d_order.get());
    order = env->d_order.get();
  }
  float4* stage = force_reset < 0 ? nullptr : env->d_stage.get();   // (sub-steps only: no render follows, the records go stale)
  if (force_reset < 0) env->stage_dirty = true;
  SRL_LAUNCH(env, 0, k_step_kernels[env->step_variant], dim3(n), dim3(k_step_variants[env->step_variant].threads), env->step_lds, st, dP,
             action, force_reset, order, stage);
  if (force_reset < 0) {   // srl_step_simulation: sub-steps only
    HIP_TRY(hipGetLastError());
    return SRL_OK;
  }
  const int L = P.c.episode_length;
  if (env->stage_dirty) {   // a test hook moved bodies since the records were made: all of them again, by the kernel
    SRL_LAUNCH(env, 2, srl_k_stage, dim3(n, (L + 3) / 4), dim3(256), 0, st, P, env->d_stage.get(), L, (const float*)nullptr,
               (const int32_t*)nullptr, (const int32_t*)nullptr);
    env->stage_dirty = false;
  }
  SRL_LAUNCH(env, 1, k_render_of_dtype[P.c.obs_dtype], dim3(n), dim3(SRL_RENDER_THREADS), env->render_lds, st, P,
             (const float4*)env->d_stage.get(), L, (uint8_t*)obs_map, (uint8_t*)obs_obj, reward, done, (const int32_t*)nullptr, (float*)nullptr);
  HIP_TRY(hipGetLastError());
  return SRL_OK;
}

// Snapshots of the header array and the blob: one contiguous blocking copy each way.  read_headers leaves the device idle
// first; every site reads the headers before it touches the blob.
template <class T> int pull(std::vector<T>& v, const T* dev, size_t count) {
  v.resize(count);
  HIP_TRY(hipMemcpy(v.data(), dev, sizeof(T) * count, hipMemcpyDeviceToHost));
  return SRL_OK;
}
template <class T> int push(T* dev, const std::vector<T>& v) {
  HIP_TRY(hipMemcpy(dev, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  return SRL_OK;
}
typedef std::vector<EnvHdr> Headers;
int read_headers(srl_env* env, std::vector<EnvHdr>& h) { HIP_TRY(hipDeviceSynchronize()); return pull(h, env->P.hdr, (size_t)env->P.c.n_envs); }
int write_headers(srl_env* env, const std::vector<EnvHdr>& h) { return push(env->P.hdr, h); }
int read_blob(srl_env* env, std::vector<float>& blob) { return pull(blob, env->P.blob, (size_t)env->P.c.n_envs * env->P.BLOB); }
int write_blob(srl_env* env, const std::vector<float>& blob) { return push(env->P.blob, blob); }

}  // namespace

extern "C" {

const char* srl_last_error(void) { return g_err; }

#ifndef SRL_BUILD_INFO
#define SRL_BUILD_INFO "SRL_BUILD_INFO<unknown|>"
#endif
// how this library was built (stackrl_amd/build.py): "SRL_BUILD_INFO<variant|hash of the sources and flags>"
const char* srl_build_info(void) { static const char info[] = SRL_BUILD_INFO; return info; }

int srl_config_default(srl_config* c) {
  if (!c) return fail(SRL_EINVAL, "null config");
  memset(c, 0, sizeof *c);
  c->n_envs = 1;
  c->episode_length = 30;            // DEFAULT_EPISODE_LENGTH, env.py:20
  c->overhead_res = 128; c->object_res = 32;
  c->object_max_dimension = 0.125f; c->max_z = 0.375f;
  c->sim_time_step = 0.01f; c->gravity = 9.8f; c->velocity_threshold = 0.01f;
  c->smooth_placing = 1; c->max_substeps = 0;
  c->metric = SRL_METRIC_IOU; c->goal_size_ratio = 0.25f; c->reward_scale = 1.0f;
  c->reward_pexp = 2; c->reward_oexp = 2;   // Stack-v0 registry: reward_params=2
  c->solver_iterations = 50; c->collision_margin = 0.001f; c->erp = 0.2f;
  c->friction_rock = 0.6f; c->friction_ground = 0.5f;
  c->linear_damping = 0.04f; c->angular_damping = 0.04f; c->warmstart = 0.1f; c->linear_slop = 1e-5f; c->residual_threshold = 1e-7f;
  c->place_at_com = 1;
  c->orientation_freedom = 0;
  c->ordering_freedom = 0;
  c->obs_dtype = SRL_DTYPE_UINT8;    // Stack-v0 registry: dtype='uint8' (envs/stack/__init__.py:4-8)
  return SRL_OK;
}

int srl_create(const srl_config* cfg, srl_env** out) {
  if (!cfg || !out) return fail(SRL_EINVAL, "null argument");
  std::unique_ptr<srl_env> env(new srl_env());   // an early return frees the handle and what it has allocated so far
  DevParams& P = env->P;
  SRL_TRY(host_params(*cfg, P));
  const int n = P.c.n_envs, res = P.c.overhead_res;
  HIP_TRY(env->hdr.alloc((size_t)n));
  HIP_TRY(env->blob.alloc((size_t)n * P.BLOB));
  HIP_TRY(env->H.alloc((size_t)n * res * res));
  HIP_TRY(env->flags.alloc(1));
  P.hdr = env->hdr.get(); P.blob = env->blob.get(); P.H = env->H.get(); P.flags = env->flags.get();
  HIP_TRY(env->d_P.alloc(1));
  HIP_TRY(env->d_reset_r.alloc(4 * (size_t)n));   // up to 4 rewards per env (metric 'all')
  HIP_TRY(env->d_stage.alloc((size_t)n * P.c.episode_length * SRL_STAGE_STRIDE));
  if (n <= SRL_ORDER_MAX_ENVS) {   // launch order of the settle kernel (srl_k_order_*): keys + permutation, owned by the handle
    HIP_TRY(env->d_order_keys.alloc((size_t)n));
    HIP_TRY(env->d_order.alloc((size_t)n));
    if (n > 8192)
      HIP_TRY(hipFuncSetAttribute((const void*)srl_k_order_sort, hipFuncAttributeMaxDynamicSharedMemorySize, SRL_ORDER_MAX_ENVS * 8));
  }
  HIP_TRY(env->d_reset_d.alloc((size_t)n));
  HIP_TRY(hipMemset(P.blob, 0, sizeof(float) * (size_t)n * P.BLOB));
  HIP_TRY(hipMemset(P.H, 0, sizeof(float) * (size_t)n * res * res));
  HIP_TRY(hipMemset(P.flags, 0, sizeof(int32_t)));
  std::vector<EnvHdr> h((size_t)n);   // (zeros)
  for (int i = 0; i < n; ++i) { h[i].done = 1; h[i].pending = -1; h[i].ncolour = -1; }   // env.py:219-220
  SRL_TRY(write_headers(env.get(), h));
  {   // codec table: one entry per float32 between FAR - max_z and FAR (6,145 at max_z = 0.375) + the empty-pixel entry
    const float nearp = SRL_FAR - P.c.max_z;
    const double span = ((double)SRL_FAR - (double)nearp) * 16384.0;
    if (!(nearp >= 512.0f && span <= 65536.0)) {
      (void)hipDeviceSynchronize();
      return fail(SRL_EINVAL, "max_z must be at most 4 (the depth codec is tabulated over the float32 lattice of 1000 - z)");
    }
    const int nt = (int)span + 1;
    HIP_TRY(env->d_codec.alloc((size_t)(nt + 3)));
    hipLaunchKernelGGL(srl_k_codec_table, dim3((nt + 3 + 255) / 256), dim3(256), 0, 0, P, env->d_codec.get(), nt);
    HIP_TRY(hipDeviceSynchronize());
    P.codec = env->d_codec.get(); P.codec_n = nt;
    uint2 row0, rowg, rowo;   // constants evaluated by the device (DevParams::h_empty ...)
    HIP_TRY(hipMemcpy(&row0, P.codec, sizeof(uint2), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&rowg, P.codec + nt + 1, sizeof(uint2), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&rowo, P.codec + nt + 2, sizeof(uint2), hipMemcpyDeviceToHost));
    memcpy(&P.h_empty, &row0.x, sizeof(float));
    P.b_empty = row0.y; P.gbyte = rowg.x; P.zbyte = rowg.y; P.obj_empty_byte = rowo.x;
    P.walk_di = (4 * SRL_RENDER_THREADS) / res; P.walk_dj = 4 * SRL_RENDER_THREADS - P.walk_di * res;
    P.res_magic = (uint32_t)(0x100000000ull / (unsigned long long)res) + 1u;
  }
  *out = env.release();
  return SRL_OK;
}

void srl_destroy(srl_env* env) {
  if (!env) return;
  (void)hipDeviceSynchronize();
  for (auto& p : env->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto& e : env->pool) (void)hipEventDestroy(e);
  delete env;   // (every device buffer is a DevBuf)
}

// Commits last: the host table, the layout and LDS sizes in a copy of P and every refusal, then the uploads into buffers of
// their own, the function attributes and the new pool's object maps; only then the handle takes buffers and parameters.  A
// failure leaves it, a table loaded earlier included, exactly as it was; meanwhile the old and the new table coexist on the device.
int srl_load_meshes(srl_env* env, const float* verts, const int32_t* vert_off, const int32_t* tris,
                    const int32_t* tri_off, const float* mass_com, int32_t n_mesh) {
  if (!env || !verts || !vert_off || !tris || !tri_off || !mass_com) return fail(SRL_EINVAL, "null argument");
  if (n_mesh < 1) return fail(SRL_EINVAL, "List of object descriptor files is empty.");   // env.py:103
  MeshTable T;
  SRL_TRY(T.build(verts, vert_off, tris, tri_off, mass_com, n_mesh));
  DevParams P = env->P;
  P.n_mesh = n_mesh; P.VS = T.vs;
  layout(P, env->concurrent_envs);
  if (P.BLOB != env->P.BLOB) return fail(SRL_EINVAL, "internal: blob layout changed");
  const size_t step_lds = sizeof(float) * (size_t)P.LDS_WORDS;
  if (step_lds > 160 * 1024) return fail(SRL_EINVAL, "episode_length x mesh size exceeds the 160 KB LDS budget");
  const size_t render_lds = render_lds_bytes(P.c.overhead_res);
  if (render_lds > 160 * 1024) return fail(SRL_EINVAL, "overhead_res exceeds the 160 KB LDS budget of the render tile (at most 176)");
  DevBuf<MeshHdr> mh; DevBuf<float4> mv, mp; DevBuf<uchar4> mt, me; DevBuf<float> objmap; DevBuf<uint8_t> objmap_u8;
  const size_t maps = (size_t)n_mesh * P.n_orient * P.c.object_res * P.c.object_res;
  HIP_TRY(mh.alloc(T.mh.size()));
  HIP_TRY(mv.alloc(T.mv.size()));
  HIP_TRY(mt.alloc(T.mt.size()));
  HIP_TRY(mp.alloc(T.mp.size()));
  HIP_TRY(objmap.alloc(maps));
  HIP_TRY(objmap_u8.alloc(maps));
  SRL_TRY(push(mh.get(), T.mh));
  SRL_TRY(push(mv.get(), T.mv));
  SRL_TRY(push(mt.get(), T.mt));
  SRL_TRY(push(mp.get(), T.mp));
  HIP_TRY(me.alloc(T.me.size()));
  SRL_TRY(push(me.get(), T.me));
  P.mh = mh.get(); P.mv = mv.get(); P.mt = mt.get(); P.mp = mp.get(); P.me = me.get();
  P.objmap = objmap.get(); P.objmap_u8 = objmap_u8.get();
  for (const auto k : k_step_kernels)
    HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)step_lds));
  HIP_TRY(hipFuncSetAttribute((const void*)srl_k_render, hipFuncAttributeMaxDynamicSharedMemorySize, (int)render_lds));
  if (P.c.obs_dtype != SRL_DTYPE_UINT8)   // (both: srl_render_heightmap runs srl_k_render whatever the observation's type)
    HIP_TRY(hipFuncSetAttribute((const void*)k_render_of_dtype[P.c.obs_dtype], hipFuncAttributeMaxDynamicSharedMemorySize, (int)render_lds));
  // K3: object maps of the whole pool, once
  hipLaunchKernelGGL(srl_k_objmap, dim3(n_mesh, P.n_orient), dim3(256), 0, 0, P, objmap.get(), objmap_u8.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());   // from here on the commit; the locals take the old table and free it on return
  env->d_mh.swap(mh); env->d_mv.swap(mv); env->d_mt.swap(mt); env->d_mp.swap(mp); env->d_me.swap(me);
  env->d_objmap.swap(objmap); env->d_objmap_u8.swap(objmap_u8);
  env->P = P; env->mesh_hash = T.hash;
  env->step_lds = step_lds; env->render_lds = render_lds; env->step_variant = step_variant_of(P, env->concurrent_envs);
  env->P_dirty = true; env->stage_dirty = true;     // (records made from another mesh table are stale)
  return SRL_OK;
}

int srl_set_concurrent_envs(srl_env* env, int32_t n_envs_on_device) {
  if (!env) return fail(SRL_EINVAL, "null env");
  if (n_envs_on_device < 0) return fail(SRL_EINVAL, "n_envs_on_device must be >= 0");
  if (env->d_mh.get()) return fail(SRL_EINVAL, "srl_set_concurrent_envs must precede srl_load_meshes");
  env->concurrent_envs = n_envs_on_device;
  return SRL_OK;
}

int srl_get_step_variant(srl_env* env, int32_t* threads, int32_t* points_per_thread, int32_t* kernel) {
  if (!env) return fail(SRL_EINVAL, "null env");
  if (!env->d_mh.get()) return fail(SRL_ENOMESH, "srl_load_meshes must be called first (it chooses the variant)");
  const StepRow& sv = k_step_variants[env->step_variant];
  if (threads) *threads = sv.threads;
  if (points_per_thread) *points_per_thread = sv.pp;
  if (kernel) *kernel = sv.reports;
  return SRL_OK;
}

int srl_set_launch_order(srl_env* env, int32_t mode) {
  if (!env) return fail(SRL_EINVAL, "null env");
  if (mode < -1 || mode > 1) return fail(SRL_EINVAL, "launch order mode must be -1 (by batch size), 0 (index order) or 1 (highest release first)");
  if (mode == 1 && !env->d_order.get()) return fail(SRL_EINVAL, "ordered launch supports at most 16,384 envs per handle");
  env->order_mode = mode;
  return SRL_OK;
}

int srl_seed(srl_env* env, uint32_t seed) {
  if (!env) return fail(SRL_EINVAL, "null env");
  env->P.seed = seed;
  env->P.sample_counter = 0;
  env->P_dirty = true;
  Headers h;   // episode counters restart
  SRL_TRY(read_headers(env, h));
  for (EnvHdr& e : h) e.episode = 0u;
  SRL_TRY(write_headers(env, h));
  HIP_TRY(hipDeviceSynchronize());
  return SRL_OK;
}

int srl_set_script(srl_env* env, const int32_t* mesh_ids, const int32_t* goal_rect) {
  if (!env || !mesh_ids || !goal_rect) return fail(SRL_EINVAL, "null argument");
  const DevParams& P = env->P;
  const int n = P.c.n_envs, L = P.c.episode_length;
  for (size_t k = 0; k < (size_t)n * L; ++k)
    if (mesh_ids[k] < 0 || mesh_ids[k] >= P.n_mesh) return fail(SRL_EINVAL, "script mesh id out of range");
  Headers h;
  SRL_TRY(read_headers(env, h));
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < L; ++k) h[i].script_ids[k] = mesh_ids[(size_t)i * L + k];
    for (int k = 0; k < 4; ++k) h[i].script_goal[k] = goal_rect[(size_t)i * 4 + k];
    h[i].has_script = 1;
  }
  SRL_TRY(write_headers(env, h));
  HIP_TRY(hipDeviceSynchronize());
  return SRL_OK;
}

int srl_reset(srl_env* env, void* obs_map, void* obs_obj, void* stream) {
  if (!env || !obs_map || !obs_obj) return fail(SRL_EINVAL, "null argument");
  // reward/done of a reset are zeros (utils.py:545-552) that the kernels write to the handle's own buffers (srl_create)
  return launch_step_render(env, nullptr, obs_map, obs_obj, env->d_reset_r.get(), env->d_reset_d.get(), (hipStream_t)stream, 1);
}

int srl_step(srl_env* env, const int64_t* action, void* obs_map, void* obs_obj, float* reward, uint8_t* done, void* stream) {
  if (!env || !action || !obs_map || !obs_obj || !reward || !done) return fail(SRL_EINVAL, "null argument");
  return launch_step_render(env, action, obs_map, obs_obj, reward, done, (hipStream_t)stream, 0);
}

int srl_step_simulation(srl_env* env, int32_t n_substeps, void* stream) {
  if (!env || n_substeps < 1 || n_substeps > 100000) return fail(SRL_EINVAL, "n_substeps must be in [1, 100000]");
  return launch_step_render(env, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream, -n_substeps);
}

int srl_set_body_state(srl_env* env, const float* poses, const float* vel) {
  if (!env) return fail(SRL_EINVAL, "null env");
  const DevParams& P = env->P;
  const int n = P.c.n_envs;
  Headers h; std::vector<float> blob;
  SRL_TRY(read_headers(env, h)); SRL_TRY(read_blob(env, blob));
  for (int i = 0; i < n; ++i) {
    float* gb = blob.data() + (size_t)i * P.BLOB;
    for (int b = 0; b < h[i].nb; ++b) {
      if (poses) {
        const float* p = poses + ((size_t)i * SRL_MAX_BODIES + b) * 8;
        for (int k = 0; k < 3; ++k) gb[P.OFF_X + 4 * b + k] = p[k];
        for (int k = 0; k < 4; ++k) gb[P.OFF_Q + 4 * b + k] = p[3 + k];
      }
      if (vel) {
        const float* p = vel + ((size_t)i * SRL_MAX_BODIES + b) * 8;
        for (int k = 0; k < 3; ++k) { gb[P.OFF_V + 8 * b + 2 * k] = p[k]; gb[P.OFF_W + 8 * b + 2 * k] = p[4 + k]; }
      }
    }
  }
  SRL_TRY(write_blob(env, blob));
  env->stage_dirty = true;
  return SRL_OK;
}

int srl_sample(srl_env* env, int64_t* action, void* stream) {
  if (!env || !action) return fail(SRL_EINVAL, "null argument");
  env->P.sample_counter += 1;
  const int n = env->P.c.n_envs;
  hipLaunchKernelGGL(srl_k_sample, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, env->P, action);
  HIP_TRY(hipGetLastError());
  return SRL_OK;
}

int srl_sync_status(srl_env* env, void* stream) {
  if (!env) return fail(SRL_EINVAL, "null env");
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  int32_t f = 0;
  HIP_TRY(hipMemcpy(&f, env->P.flags, sizeof f, hipMemcpyDeviceToHost));
  if (f) { const int32_t zero = 0; HIP_TRY(hipMemcpy(env->P.flags, &zero, sizeof zero, hipMemcpyHostToDevice)); }
  if (f & 1) return fail(SRL_EINVAL_ACTION, "Invalid action.");
  if (f & 2) return fail(SRL_ESIM_DIVERGED, "Maximum number of simulator steps reached. This may be caused by incorrect behaviour due to a large time step value");
  if (f & 4) return fail(SRL_ESIM_DIVERGED, "More close rock pairs than manifold slots in some env (SRL_ST_PAIR_OVERFLOW): the step is not valid");
  if (f & SRL_FLAG_STATE_INDEX) return fail(SRL_EINVAL, "srl_state_get / srl_state_set: an env index outside the handle, or a negative record index (that pair was skipped)");
  return SRL_OK;
}

int srl_get_state(srl_env* env, float* poses, int32_t* n_bodies, int32_t* substeps, int32_t* status) {
  if (!env) return fail(SRL_EINVAL, "null env");
  const DevParams& P = env->P;
  const int n = P.c.n_envs;
  Headers h; std::vector<float> blob;
  SRL_TRY(read_headers(env, h));
  if (poses) {
    SRL_TRY(read_blob(env, blob));
    memset(poses, 0, sizeof(float) * (size_t)n * SRL_MAX_BODIES * 8);
  }
  for (int i = 0; i < n; ++i) {
    if (poses) {
      const float* gb = blob.data() + (size_t)i * P.BLOB;
      float* p = poses + (size_t)i * SRL_MAX_BODIES * 8;
      for (int b = 0; b < h[i].nb; ++b) {
        for (int k = 0; k < 3; ++k) p[b * 8 + k] = gb[P.OFF_X + 4 * b + k];
        for (int k = 0; k < 4; ++k) p[b * 8 + 3 + k] = gb[P.OFF_Q + 4 * b + k];
        p[b * 8 + 7] = (float)((const int32_t*)gb)[P.OFF_MESH + b];
      }
    }
    if (n_bodies) n_bodies[i] = h[i].nb;
    if (substeps) { substeps[2 * i] = h[i].substeps[0]; substeps[2 * i + 1] = h[i].substeps[1]; }
    if (status) status[i] = h[i].status;
  }
  return SRL_OK;
}

int srl_get_sweeps(srl_env* env, int32_t* sweeps) {
  if (!env || !sweeps) return fail(SRL_EINVAL, "null argument");
  Headers h;
  SRL_TRY(read_headers(env, h));
  for (size_t i = 0; i < h.size(); ++i) sweeps[i] = h[i].sweeps;
  return SRL_OK;
}

int srl_get_velocities(srl_env* env, float* vel) {
  if (!env || !vel) return fail(SRL_EINVAL, "null argument");
  const DevParams& P = env->P;
  const int n = P.c.n_envs;
  Headers h; std::vector<float> blob;
  SRL_TRY(read_headers(env, h)); SRL_TRY(read_blob(env, blob));
  memset(vel, 0, sizeof(float) * (size_t)n * SRL_MAX_BODIES * 8);
  for (int i = 0; i < n; ++i) {
    const float* gb = blob.data() + (size_t)i * P.BLOB;
    float* p = vel + (size_t)i * SRL_MAX_BODIES * 8;
    for (int b = 0; b < h[i].nb; ++b)
      for (int k = 0; k < 3; ++k) { p[b * 8 + k] = gb[P.OFF_V + 8 * b + 2 * k]; p[b * 8 + 4 + k] = gb[P.OFF_W + 8 * b + 2 * k]; }
  }
  return SRL_OK;
}

int srl_get_contacts(srl_env* env, float* max_penetration, int32_t* n_points) {
  if (!env || !max_penetration || !n_points) return fail(SRL_EINVAL, "null argument");
  const int n = env->P.c.n_envs;
  DevBuf<float> d_mp; DevBuf<int32_t> d_np;
  HIP_TRY(d_mp.alloc((size_t)n));
  HIP_TRY(d_np.alloc((size_t)n));
  hipLaunchKernelGGL(srl_k_contacts, dim3((n + 63) / 64), dim3(64), 0, 0, env->P, d_mp.get(), d_np.get());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(max_penetration, d_mp.get(), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(n_points, d_np.get(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  return SRL_OK;
}

int srl_get_maps(srl_env* env, float* height, float* object_map, int32_t* goal_rect) {
  if (!env) return fail(SRL_EINVAL, "null env");
  const DevParams& P = env->P;
  const int n = P.c.n_envs, res = P.c.overhead_res, r = P.c.object_res;
  Headers h;
  SRL_TRY(read_headers(env, h));
  if (height) HIP_TRY(hipMemcpy(height, P.H, sizeof(float) * (size_t)n * res * res, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) {
    if (goal_rect) for (int k = 0; k < 4; ++k) goal_rect[4 * i + k] = h[i].goal[k];
    if (object_map) {
      const size_t per = (size_t)P.n_orient * r * r;   // every observable orientation of one rock
      // the pending rock, or with ordering freedom every rock still unplaced, then empty maps (observer.py:310-327)
      const int shown = P.c.ordering_freedom ? P.c.episode_length : 1;
      for (int k = 0; k < shown; ++k) {
        float* o = object_map + ((size_t)i * shown + k) * per;
        const int m = P.c.ordering_freedom ? (k < h[i].list_pos ? h[i].ids[k] : -1) : h[i].pending;
        if (m >= 0) {
          HIP_TRY(hipMemcpy(o, P.objmap + (size_t)m * per, sizeof(float) * per, hipMemcpyDeviceToHost));
        } else {
          const float e0 = empty_object_elevation(P);
          for (size_t kk = 0; kk < per; ++kk) o[kk] = e0;
        }
      }
    }
  }
  return SRL_OK;
}

int srl_get_object_map(srl_env* env, int32_t mesh_id, float* object_map) {
  if (!env || !object_map) return fail(SRL_EINVAL, "null argument");
  if (!env->d_objmap.get()) return fail(SRL_ENOMESH, "srl_load_meshes must be called first");
  if (mesh_id < 0 || mesh_id >= env->P.n_mesh) return fail(SRL_EINVAL, "mesh id out of range");
  const size_t per = (size_t)env->P.n_orient * env->P.c.object_res * env->P.c.object_res;
  HIP_TRY(hipMemcpy(object_map, env->P.objmap + (size_t)mesh_id * per, sizeof(float) * per, hipMemcpyDeviceToHost));
  return SRL_OK;
}

int srl_get_stage_records(srl_env* env, float* records, int64_t n_floats) {
  if (!env || !records) return fail(SRL_EINVAL, "null argument");
  const int64_t need = (int64_t)env->P.c.n_envs * env->P.c.episode_length * SRL_STAGE_STRIDE * 4;
  if (n_floats != need) return fail(SRL_EINVAL, "records must hold n_envs x episode_length x SRL_STAGE_STRIDE x 4 floats");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(records, env->d_stage.get(), sizeof(float) * (size_t)need, hipMemcpyDeviceToHost));
  return SRL_OK;
}

int32_t srl_stage_record_stride(void) { return SRL_STAGE_STRIDE; }

int srl_render_heightmap(srl_env* env, const float* poses, const int32_t* mesh_ids, const int32_t* n_bodies,
                         float* height, void* stream) {
  if (!env || !poses || !mesh_ids || !n_bodies || !height) return fail(SRL_EINVAL, "null argument");
  if (!env->d_mh.get()) return fail(SRL_ENOMESH, "srl_load_meshes must be called first");
  hipStream_t st = (hipStream_t)stream;
  const int n = env->P.c.n_envs;
  if (!env->d_stage_ext.get()) HIP_TRY(env->d_stage_ext.alloc((size_t)n * SRL_MAX_BODIES * SRL_STAGE_STRIDE));
  SRL_LAUNCH(env, 2, srl_k_stage, dim3(n, SRL_MAX_BODIES / 4), dim3(256), 0, st, env->P, env->d_stage_ext.get(), SRL_MAX_BODIES, poses,
             mesh_ids, n_bodies);
  SRL_LAUNCH(env, 1, srl_k_render, dim3(n), dim3(SRL_RENDER_THREADS), env->render_lds, st, env->P, (const float4*)env->d_stage_ext.get(),
             SRL_MAX_BODIES, (uint8_t*)nullptr, (uint8_t*)nullptr, (float*)nullptr, (uint8_t*)nullptr, n_bodies, height);
  HIP_TRY(hipGetLastError());
  return SRL_OK;
}

int srl_render_rgb(srl_env* env, int32_t dtype, void* overhead, void* object, void* stream) {
  if (!env) return fail(SRL_EINVAL, "null env");
  if (dtype != SRL_VIEW_F64 && dtype != SRL_VIEW_U8) return fail(SRL_EINVAL, "srl_render_rgb: dtype must be 0 (float64) or 1 (uint8)");
  if (!env->d_mh.get()) return fail(SRL_ENOMESH, "srl_load_meshes must be called first");
  if (!overhead && !object) return SRL_OK;
  const DevParams& P = env->P;
  ViewParams V;
  V.H = P.H; V.objmap = P.objmap; V.hdr = P.hdr;
  V.res = P.c.overhead_res; V.r = P.c.object_res; V.n_orient = P.n_orient; V.ordering = P.c.ordering_freedom;
  V.obj_empty = empty_object_elevation(P);
  const dim3 grid(P.c.n_envs), block(SRL_VIEW_THREADS);
  if (dtype == SRL_VIEW_F64) hipLaunchKernelGGL(srl_k_view, grid, block, 0, (hipStream_t)stream, V, (double*)overhead, (double*)object);
  else hipLaunchKernelGGL(srl_k_view_u8, grid, block, 0, (hipStream_t)stream, V, (uint8_t*)overhead, (uint8_t*)object);
  HIP_TRY(hipGetLastError());
  return SRL_OK;
}

int srl_render_camera(srl_env* env, const srl_camera* cam, const float* poses, const int32_t* mesh_ids, const int32_t* n_bodies,
                      const int32_t* goal_rect, uint8_t* rgb, float* depth, int32_t* ids, void* stream) {
  if (!env || !cam) return fail(SRL_EINVAL, "srl_render_camera: null argument");
  if (cam->width < 1 || cam->width > SRL_CAM_MAX_SIDE || cam->height < 1 || cam->height > SRL_CAM_MAX_SIDE)
    return fail(SRL_EINVAL, "srl_render_camera: width and height must be in 1 .. 1024");
  {
    const float* f = cam->eye;   // the 23 floats of the struct, eye .. sky_rgb
    static_assert(offsetof(srl_camera, width) == 23 * sizeof(float), "srl_camera: 23 floats, then the ints");
    for (int k = 0; k < 23; ++k)
      if (!isfinite(f[k])) return fail(SRL_EINVAL, "srl_render_camera: the camera holds a non-finite value");
    const double ff = (double)cam->fwd[0] * cam->fwd[0] + (double)cam->fwd[1] * cam->fwd[1] + (double)cam->fwd[2] * cam->fwd[2];
    const double ll = (double)cam->light[0] * cam->light[0] + (double)cam->light[1] * cam->light[1] + (double)cam->light[2] * cam->light[2];
    if (fabs(sqrt(ff) - 1.0) > 1e-3 || fabs(sqrt(ll) - 1.0) > 1e-3)
      return fail(SRL_EINVAL, "srl_render_camera: fwd and light must be unit vectors (to 1e-3)");
  }
  const int given = (poses != nullptr) + (mesh_ids != nullptr) + (n_bodies != nullptr) + (goal_rect != nullptr);
  if (given != 0 && given != 4)
    return fail(SRL_EINVAL, "srl_render_camera: the scene pointers (poses, mesh ids, body counts, goal rectangles) must be all set or all NULL");
  if (!rgb && !depth && !ids) return fail(SRL_EINVAL, "srl_render_camera: all outputs are NULL");
  if (!env->d_mh.get()) return fail(SRL_ENOMESH, "srl_load_meshes must be called first");
  const DevParams& P = env->P;
  CamParams C;
  C.cam = *cam;
  C.hdr = P.hdr; C.blob = P.blob; C.mh = P.mh; C.mp = P.mp;
  C.poses = poses; C.mesh_ids = mesh_ids; C.n_bodies = n_bodies; C.goal = goal_rect;
  C.BLOB = P.BLOB; C.OFF_X = P.OFF_X; C.OFF_Q = P.OFF_Q; C.OFF_MESH = P.OFF_MESH; C.n_mesh = P.n_mesh;
  C.max_bodies = given ? SRL_MAX_BODIES : P.c.episode_length;
  C.px = P.px; C.sx = (float)P.c.overhead_res * P.px; C.sy = C.sx;
  C.tiles_x = (cam->width + SRL_CAM_TW - 1) / SRL_CAM_TW;
  C.tiles = C.tiles_x * ((cam->height + SRL_CAM_TH - 1) / SRL_CAM_TH);
  C.rgb = rgb; C.depth = depth; C.ids = ids;
  const long long blocks = (long long)C.tiles * P.c.n_envs;
  if (blocks > 0x7fffffffLL) return fail(SRL_EINVAL, "srl_render_camera: more than 2^31 - 1 tiles in one call");
  hipLaunchKernelGGL(srl_k_camera, dim3((unsigned)blocks), dim3(SRL_CAM_THREADS), 0, (hipStream_t)stream, C);
  HIP_TRY(hipGetLastError());
  return SRL_OK;
}

// ---- state records (state.hip)

int srl_state_layout(const srl_config* cfg, int64_t* words, int64_t* part_offsets) {
  if (!cfg) return fail(SRL_EINVAL, "srl_state_layout: null config");
  DevParams P;
  SRL_TRY(host_params(*cfg, P));   // (BLOB depends on episode_length alone)
  const StateLayout s = state_layout(P);
  if (words) *words = s.words;
  if (part_offsets) for (int k = 0; k < 4; ++k) part_offsets[k] = s.off[k];
  return SRL_OK;
}

int srl_state_signature(srl_env* env, uint64_t* signature) {
  if (!signature) return fail(SRL_EINVAL, "srl_state_signature: null output");
  if (!env) return fail(SRL_EINVAL, "srl_state_signature: null env");
  if (!env->d_mh.get()) return fail(SRL_ENOMESH, "srl_load_meshes must be called first (the mesh table is part of the signature)");
  const DevParams& P = env->P;
  const srl_config& c = P.c;
  const StateLayout s = state_layout(P);
  uint64_t h = fnv1a(&s, sizeof s);
  const int64_t hdr_bytes = (int64_t)sizeof(EnvHdr);
  h = fnv1a(&hdr_bytes, sizeof hdr_bytes, h);
  h = fnv1a(&P.n_mesh, sizeof P.n_mesh, h);
  h = fnv1a(&env->mesh_hash, sizeof env->mesh_hash, h);
  // the fields that shape the state or the kernels' reading of it: the counts and resolutions, the metres a pixel and an
  // elevation stand for, what the reward memory holds, the frame the poses are in, the observation the records render to.
  // n_envs and env_index_offset are the handle's; the solver and physics parameters may differ between handles.
  const int32_t ints[] = {c.episode_length, c.overhead_res, c.object_res, c.metric, c.reward_pexp, c.reward_oexp, c.place_at_com,
                          c.orientation_freedom, c.ordering_freedom, c.obs_dtype};
  const float floats[] = {c.object_max_dimension, c.max_z, c.goal_size_ratio, c.reward_scale};
  h = fnv1a(ints, sizeof ints, h);
  h = fnv1a(floats, sizeof floats, h);
  const char* info = srl_build_info();   // "SRL_BUILD_INFO<variant|hash>": the hash of the sources
  const char* bar = strchr(info, '|');
  h = fnv1a(bar ? bar : info, strlen(bar ? bar : info), h);
  *signature = h;
  return SRL_OK;
}

// the grid of a state kernel: x = (env, record) pairs, y = chunks of a record, about SRL_STATE_BLOCKS workgroups in all (a
// bandwidth kernel), both dimensions stride
static void state_launch_shape(const srl_env* env, int n, StateParts& S, dim3& grid) {
  const DevParams& P = env->P;
  const StateLayout s = state_layout(P);
  S.hdr = (uint4*)P.hdr; S.blob = (uint4*)P.blob; S.H = (uint4*)P.H; S.stage = (uint4*)env->d_stage.get(); S.flags = P.flags;
  S.q_hdr = (int32_t)(s.size[0] / 4); S.q_blob = (int32_t)(s.size[1] / 4); S.q_H = (int32_t)(s.size[2] / 4); S.q_stage = (int32_t)(s.size[3] / 4);
  S.n_envs = P.c.n_envs;
  const int rounds = (int)((s.words / 4 + SRL_STATE_THREADS - 1) / SRL_STATE_THREADS);
  const int gx = n < SRL_STATE_BLOCKS ? n : SRL_STATE_BLOCKS;
  int gy = SRL_STATE_BLOCKS / gx;
  if (gy > rounds) gy = rounds;
  grid = dim3(gx, gy < 1 ? 1 : gy);
}

int srl_state_get(srl_env* env, const int32_t* idx_dev, int32_t n, void* records_dev, uint32_t* seed, uint32_t* sample_counter,
                  void* stream) {
  if (!records_dev) return fail(SRL_EINVAL, "srl_state_get: null records buffer");
  if (n < 1) return fail(SRL_EINVAL, "srl_state_get: n must be at least 1");
  if (!env) return fail(SRL_EINVAL, "srl_state_get: null env");
  if (!env->d_mh.get()) return fail(SRL_ENOMESH, "srl_load_meshes must be called first");
  if (!idx_dev && n != env->P.c.n_envs) return fail(SRL_EINVAL, "srl_state_get: without indexes n must be the handle's n_envs");
  if (env->stage_dirty)
    return fail(SRL_EINVAL, "srl_state_get: the staged records are stale (no step since srl_load_meshes, srl_set_body_state, srl_kick or srl_step_simulation): step first");
  StateParts S; dim3 grid;
  state_launch_shape(env, n, S, grid);
  hipLaunchKernelGGL(srl_k_state_get, grid, dim3(SRL_STATE_THREADS), 0, (hipStream_t)stream, S, idx_dev, (int)n, (uint4*)records_dev);
  HIP_TRY(hipGetLastError());
  if (seed) *seed = env->P.seed;
  if (sample_counter) *sample_counter = env->P.sample_counter;
  return SRL_OK;
}

int srl_state_set(srl_env* env, uint64_t signature, const int32_t* dst_idx_dev, const int32_t* src_rec_dev, int32_t n,
                  const void* records_dev, void* stream) {
  if (!records_dev) return fail(SRL_EINVAL, "srl_state_set: null records buffer");
  if (n < 1) return fail(SRL_EINVAL, "srl_state_set: n must be at least 1");
  if (!env) return fail(SRL_EINVAL, "srl_state_set: null env");
  uint64_t own = 0;
  const int rc = srl_state_signature(env, &own);
  if (rc) return rc;
  if (signature != own)
    return fail(SRL_EINVAL, "srl_state_set: the records' signature is not this handle's (another record layout, mesh pool, configuration or library build)");
  if (n > env->P.c.n_envs) return fail(SRL_EINVAL, "srl_state_set: more destinations than envs (they must be distinct)");
  StateParts S; dim3 grid;
  state_launch_shape(env, n, S, grid);
  hipLaunchKernelGGL(srl_k_state_set, grid, dim3(SRL_STATE_THREADS), 0, (hipStream_t)stream, S, dst_idx_dev, src_rec_dev, (int)n,
                     (uint4*)const_cast<void*>(records_dev));
  HIP_TRY(hipGetLastError());
  // the whole batch in index order brings its staged records along; after a partial set a stale batch stays stale (the next
  // step makes every record again from the poses, the restored ones included)
  if (!dst_idx_dev && n == env->P.c.n_envs) env->stage_dirty = false;
  return SRL_OK;
}

int srl_state_set_rng(srl_env* env, uint32_t seed, uint32_t sample_counter) {
  if (!env) return fail(SRL_EINVAL, "srl_state_set_rng: null env");
  env->P.sample_counter = sample_counter;   // (read from the host copy only: srl_sample passes it by value)
  if (seed != env->P.seed) {   // the settle kernels read the seed from the device copy of the parameters: as after srl_seed, the
    // device is left idle and the next launch uploads the block
    HIP_TRY(hipDeviceSynchronize());
    env->P.seed = seed;
    env->P_dirty = true;
  }
  return SRL_OK;
}

// ---- contact points (contacts.hip)

int32_t srl_contact_row_words(void) { return SRL_CONTACT_ROW_WORDS; }

int srl_contact_max_points(srl_env* env, int32_t* max_points) {
  if (!env) return fail(SRL_EINVAL, "srl_contact_max_points: null env");
  if (!max_points) return fail(SRL_EINVAL, "srl_contact_max_points: null output");
  *max_points = SRL_GMAXP * env->P.c.episode_length + 4 * env->P.NS;   // every ground manifold and every slot full
  return SRL_OK;
}

int srl_contact_points(srl_env* env, int32_t last_only, int32_t capacity, int32_t* count_dev, int32_t* bodies_dev, float* rows_dev,
                       float* wrench_dev, void* stream) {
  if (!env) return fail(SRL_EINVAL, "srl_contact_points: null env");
  if (capacity < 1) return fail(SRL_EINVAL, "srl_contact_points: capacity must be at least 1");   // (first: buffers of no rows are null)
  if (last_only != 0 && last_only != 1) return fail(SRL_EINVAL, "srl_contact_points: last_only must be 0 or 1");
  if (!count_dev || !bodies_dev || !rows_dev) return fail(SRL_EINVAL, "srl_contact_points: null output (count, bodies and rows are required)");
  if (((uintptr_t)bodies_dev & 7) || ((uintptr_t)rows_dev & 15) || ((uintptr_t)wrench_dev & 15))
    return fail(SRL_EINVAL, "srl_contact_points: bodies must be 8-byte aligned, rows and wrench 16-byte aligned");
  if (!env->d_mh.get()) return fail(SRL_ENOMESH, "srl_contact_points: srl_load_meshes must be called first");
  const DevParams& P = env->P;
  static_assert(SRL_NSLOT_MAX >= 128, "the kernel's slot table holds every slot of nslots()");
  ContactParams C;
  C.hdr = P.hdr; C.blob = P.blob; C.mh = P.mh; C.mv = P.mv;
  C.BLOB = P.BLOB; C.OFF_X = P.OFF_X; C.OFF_Q = P.OFF_Q; C.OFF_MESH = P.OFF_MESH; C.OFF_GM = P.OFF_GM; C.OFF_MAN = P.OFF_MAN;
  C.OFF_POS = P.OFF_POS; C.NS = P.NS; C.NP = P.NP; C.L = P.c.episode_length; C.n_mesh = P.n_mesh;
  C.dt = P.c.sim_time_step;
  C.last_only = last_only; C.capacity = capacity;
  C.count = count_dev; C.bodies = bodies_dev; C.rows = rows_dev; C.wrench = wrench_dev;
  SRL_LAUNCH(env, 4, srl_k_contact_points, dim3(P.c.n_envs), dim3(SRL_CONTACT_THREADS), 0, (hipStream_t)stream, C);
  HIP_TRY(hipGetLastError());
  return SRL_OK;
}

// ---- push test (push.hip)

static PushParams push_params(const srl_env* env) {
  const DevParams& P = env->P;
  PushParams C;
  C.hdr = P.hdr; C.blob = P.blob;
  C.BLOB = P.BLOB; C.OFF_X = P.OFF_X; C.OFF_Q = P.OFF_Q; C.OFF_V = P.OFF_V; C.OFF_PX = P.OFF_PX; C.OFF_PQ = P.OFF_PQ;
  C.OFF_MESH = P.OFF_MESH; C.L = P.c.episode_length;
  return C;
}

int srl_poses(srl_env* env, float* poses_dev, int32_t* n_bodies_dev, void* stream) {
  if (!env) return fail(SRL_EINVAL, "srl_poses: null env");
  if (!poses_dev || !n_bodies_dev) return fail(SRL_EINVAL, "srl_poses: null output (poses and n_bodies are required)");
  if ((uintptr_t)poses_dev & 15) return fail(SRL_EINVAL, "srl_poses: poses must be 16-byte aligned");
  SRL_LAUNCH(env, 4, srl_k_poses, dim3(env->P.c.n_envs), dim3(SRL_PUSH_THREADS), 0, (hipStream_t)stream, push_params(env), poses_dev,
             n_bodies_dev);
  HIP_TRY(hipGetLastError());
  return SRL_OK;
}

int srl_kick(srl_env* env, const float* dv_dev, int32_t per_body, int32_t select, void* stream) {
  if (!env) return fail(SRL_EINVAL, "srl_kick: null env");
  if (!dv_dev) return fail(SRL_EINVAL, "srl_kick: null increments");
  if ((uintptr_t)dv_dev & 15) return fail(SRL_EINVAL, "srl_kick: the increments must be 16-byte aligned");
  if (per_body != 0 && per_body != 1) return fail(SRL_EINVAL, "srl_kick: per_body must be 0 or 1");
  if (select < SRL_KICK_LAST || select >= env->P.c.episode_length)
    return fail(SRL_EINVAL, "srl_kick: select must be SRL_KICK_ALL, SRL_KICK_LAST or a body slot below episode_length");
  SRL_LAUNCH(env, 4, srl_k_kick, dim3(env->P.c.n_envs), dim3(SRL_PUSH_THREADS), 0, (hipStream_t)stream, push_params(env), dv_dev,
             (int)per_body, (int)select);
  HIP_TRY(hipGetLastError());
  env->stage_dirty = true;   // as after srl_set_body_state: bodies change behind the staged records' back
  return SRL_OK;
}

int srl_pose_distances(srl_env* env, const float* ref_dev, const int32_t* ref_nb_dev, float tol_p, float tol_o, float* rows_dev,
                       float* summary_dev, void* stream) {
  if (!env) return fail(SRL_EINVAL, "srl_pose_distances: null env");
  if (!rows_dev || !summary_dev) return fail(SRL_EINVAL, "srl_pose_distances: null output (rows and summary are required)");
  if (((uintptr_t)ref_dev & 15) || ((uintptr_t)rows_dev & 15) || ((uintptr_t)summary_dev & 15))
    return fail(SRL_EINVAL, "srl_pose_distances: the reference, rows and summary must be 16-byte aligned");
  SRL_LAUNCH(env, 4, srl_k_pose_distances, dim3(env->P.c.n_envs), dim3(SRL_PUSH_THREADS), 0, (hipStream_t)stream, push_params(env), ref_dev,
             ref_nb_dev, tol_p, tol_o, rows_dev, summary_dev);
  HIP_TRY(hipGetLastError());
  return SRL_OK;
}

#ifdef SRL_STAMPS
// diagnostic build only: `count` tick counters per env, from the header field at `offset`, to the host array [n][count]
static int debug_field(srl_env* env, long long* out, size_t offset, int count) {
  Headers h;
  SRL_TRY(read_headers(env, h));
  for (size_t i = 0; i < h.size(); ++i) memcpy(out + count * i, (const char*)&h[i] + offset, sizeof(long long) * count);
  return SRL_OK;
}
static_assert(offsetof(EnvHdr, stamps2) == offsetof(EnvHdr, stamps) + 8 * sizeof(long long), "stamps2 follows stamps");
int srl_debug_stamps(srl_env* env, long long* out) { return debug_field(env, out, offsetof(EnvHdr, stamps), 8 + 4); }   // (100 MHz wall clock)
int srl_debug_hwid(srl_env* env, long long* out) { return debug_field(env, out, offsetof(EnvHdr, hwid), 2); }
int srl_debug_diag(srl_env* env, long long* out) { return debug_field(env, out, offsetof(EnvHdr, diag), 6); }
int srl_debug_rstamps(srl_env* env, long long* out, int reset) {
  Headers h;
  SRL_TRY(read_headers(env, h));
  for (size_t i = 0; i < h.size(); ++i) for (int k = 0; k < 8; ++k) { out[8 * i + k] = h[i].rstamps[k]; if (reset) h[i].rstamps[k] = 0; }
  if (reset) SRL_TRY(write_headers(env, h));
  return SRL_OK;
}
#endif

int srl_set_profiling(srl_env* env, int32_t enable) {
  if (!env) return fail(SRL_EINVAL, "null env");
  env->profiling = enable != 0;
  return SRL_OK;
}

int srl_get_kernel_times(srl_env* env, float* ms3, int32_t* launches3) {
  if (!env) return fail(SRL_EINVAL, "null env");
  HIP_TRY(hipDeviceSynchronize());
  for (auto& p : env->pending) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { env->acc_ms[p.which] += ms; env->acc_n[p.which] += 1; }
    env->pool.push_back(p.a); env->pool.push_back(p.b);
  }
  env->pending.clear();
  for (int k = 0; k < 3; ++k) {
    if (ms3) ms3[k] = env->acc_ms[k];
    if (launches3) launches3[k] = env->acc_n[k];
    env->acc_ms[k] = 0.0f; env->acc_n[k] = 0;
  }
  return SRL_OK;
}

// the same for the two kernels of the ordered launch (srl_k_order_keys + srl_k_order_sort: two launches per ordered step),
// which run before the settle kernel and are not part of its time
int srl_get_order_kernel_times(srl_env* env, float* ms, int32_t* launches) {
  if (!env) return fail(SRL_EINVAL, "null env");
  if (!env->pending.empty()) return fail(SRL_EINVAL, "call srl_get_kernel_times first (it collects the pending events)");
  if (ms) *ms = env->acc_ms[3];
  if (launches) *launches = env->acc_n[3];
  env->acc_ms[3] = 0.0f; env->acc_n[3] = 0;
  return SRL_OK;
}

// Test hook: the keys and the permutation of the latest ordered launch (settle.hip srl_k_order_*): keys[i] = (inverted release
// height bits << 32 | i) of env i, order[k] = the env workgroup k served.  Synchronises the device.
int srl_get_launch_order(srl_env* env, unsigned long long* keys, int32_t* order) {
  if (!env || !keys || !order) return fail(SRL_EINVAL, "null argument");
  if (!env->d_order.get()) return fail(SRL_EINVAL, "this handle has no launch-order buffers (more than 16,384 envs)");
  const int n = env->P.c.n_envs;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(keys, env->d_order_keys.get(), sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(order, env->d_order.get(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  return SRL_OK;
}

}  // extern "C"
