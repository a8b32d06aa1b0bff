/* stackrl_hip.h — C-ABI of libstackrl_hip.so, the MI355X-native batched Stack-v0 env step.
 *
 * This is the drop-in boundary for the reference's `stackrl.envs.make('Stack-v0', n_parallel=B)`
 * object (stackrl/envs/utils.py:185-300 `Env`, :302-576 `ParallelEnv`): one handle owns B
 * independent envs on one GPU; `srl_step` replaces the `conn.send((STEP, a))` / `conn.recv()`
 * fan-out (utils.py:468-486, :540-543, :554-566) plus everything each worker process runs for it
 * (`StackEnv.step` env.py:233-264 -> `Observer.pose` observer.py:392-421 -> `Simulator.step`
 * simulator.py:190-258 -> `Observer.__call__` observer.py:249-277 -> `Rewarder.__call__`
 * rewarder.py:144-179 -> `StackEnv.observation` env.py:225-231).
 *
 * Conventions
 *  - plain C, no torch / HIP types in the signatures; `stream` is a hipStream_t passed as void*
 *    (NULL = the null stream).
 *  - "dev" pointers are device memory owned by the caller; "host" pointers are host memory.
 *  - every function returns an SRL_* code (include/srl_types.h); `srl_last_error()` gives the
 *    message of the calling thread's last failure.
 *  - `srl_reset/srl_step/srl_sample` only enqueue work on `stream` and return; the caller's
 *    buffers are valid when the stream reaches that point.  No device allocation, free or blocking
 *    copy happens in them in steady state (the first launch after srl_create / srl_load_meshes /
 *    srl_seed uploads the parameter block with one blocking copy; with srl_set_profiling on, HIP
 *    events are created on demand).
 *  - a handle is not thread-safe; distinct handles are independent: they share no device or host
 *    state (no process-wide tables, no common scratch buffers), so handles on different streams may
 *    step concurrently (`tests/test_parity_gpu.py::test_two_handles_on_two_streams_*`).
 */
#ifndef STACKRL_HIP_H_
#define STACKRL_HIP_H_

#include "srl_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srl_env srl_env;

/* Stack-v0 defaults: env.py:28-51 under the registry kwargs of envs/stack/__init__.py:4-8. */
int srl_config_default(srl_config* cfg);

/* `envs.make(...)` / `ParallelEnv.__init__` + `start` (utils.py:311-448): allocates all device state
 * for cfg->n_envs envs on the current HIP device. */
int srl_create(const srl_config* cfg, srl_env** out);
/* `ParallelEnv.terminate` (utils.py:450-466). */
void srl_destroy(srl_env* env);
const char* srl_last_error(void);

/* Mesh pool = the URDF list `data.generated(name='[5-9]?')` (envs/data/__init__.py:39-83) preloaded
 * once instead of `loadURDF` per step (simulator.py:297-308).  Host pointers, OBJ/URDF link frame:
 * verts float[vert_off[n_mesh]][3]; tris int32[tri_off[n_mesh]][3] per-mesh local, outward CCW;
 * mass_com float[n_mesh][4] = mass, inertial origin xyz (template.urdf:8-9). */
int srl_load_meshes(srl_env* env, const float* verts, const int32_t* vert_off, const int32_t* tris,
                    const int32_t* tri_off, const float* mass_com, int32_t n_mesh);

/* `ParallelEnv.seed` (utils.py:522-532) / `StackEnv.seed` (env.py:341-346): env i uses
 * seed + env_index_offset + i (mod 2^32) as the key of its counter RNG; episode counters restart. */
int srl_seed(srl_env* env, uint32_t seed);

/* Explicit episode script for the NEXT reset of every env (host pointers): mesh_ids int32[n][L],
 * goal_rect int32[n][4] = (u, v, h, w).  Stands in for the reference's RNG streams
 * (env.py:268-272, rewarder.py:211-259), which are gym-version dependent. */
int srl_set_script(srl_env* env, const int32_t* mesh_ids, const int32_t* goal_rect);

/* `ParallelEnv.reset` (utils.py:488-503, :545-552): obs_map u8[n][H][W][2], obs_obj u8[n][h][w][1].
 * With orientation_freedom = k > 0 (`TestStackEnv`, env.py:443-470) obs_obj is u8[n][2^k][h][w][1]: one object map per
 * observable orientation (the overhead map is returned once, not 2^k copies as env.py:472-480 stacks them).
 * With ordering_freedom = 1 (`TestSimulator`, simulator.py:343-378) obs_obj is u8[n][L * 2^k][h][w][1]: the maps of the
 * rocks still unplaced first (rock-major, orientation-minor, observer.py:310-327), empty maps after them — the fixed-size
 * form of the reference's shrinking list (env.py:596-608).
 * Element type: "u8" above is cfg->obs_dtype's (srl_config, SRL_DTYPE_*; the reference's `dtype`, env.py:168-180), so the
 * per-env strides of both buffers are those counts times the element size: uint16 / float16 2 bytes, uint32 / float32 4,
 * uint64 / float64 8.  Integer types hold x * (2^k - 1) / max(max_z, object_max_dimension) in float32, truncated as numpy
 * does on x86-64 (a height equal to that maximum is 0 in uint32 / uint64: float32(2^k - 1) = 2^k wraps, DESIGN.md
 * section 5); float types hold the float32 map values (float16 rounded to nearest even).  The same holds for srl_step. */
int srl_reset(srl_env* env, void* obs_map_dev, void* obs_obj_dev, void* stream);

/* `ParallelEnv.step` (utils.py:468-486): action int64[n]; reward float[n] (float[n][4] with metric 'all' = IoU, OR, DIoU,
 * DOR; float[n][2] with 'eval' = IoU, AD: the dict of rewarder.py:147-158 as columns); done uint8[n].
 * Auto-reset semantics of env.py:235-236 are kept: a step on a finished env returns the reset
 * observation, reward 0, done 0.  With orientation_freedom > 0 the action is orientation * A + pixel
 * (the reference's `(index, action)` tuple, env.py:485-494) and the rock is placed in that orientation.  With
 * ordering_freedom the index also names the rock: action = (rock * 2^k + orientation) * A + pixel, rock counted among
 * those still unplaced (it is popped from the list, simulator.py:372-378); an index past the maps on show is an invalid
 * action (env.py:484); the episode ends when no rock is left (env.py:513-514). */
int srl_step(srl_env* env, const int64_t* action_dev, void* obs_map_dev, void* obs_obj_dev,
             float* reward_dev, uint8_t* done_dev, void* stream);

/* `ParallelEnv.sample` (utils.py:534-538): uniform actions in [0, A), int64[n] on the device ([0, maps on show * A) for
 * `TestStackEnv`). */
int srl_sample(srl_env* env, int64_t* action_dev, void* stream);

/* Blocks until `stream` is idle and reports what the reference would have raised during the steps
 * since the last call: SRL_EINVAL_ACTION ("Invalid action.", env.py:238), SRL_ESIM_DIVERGED
 * (simulator.py:221-224 / :242-245), else SRL_OK. */
int srl_sync_status(srl_env* env, void* stream);

/* Telemetry (host pointers, synchronises the device; any pointer may be NULL):
 * `Simulator.poses` (simulator.py:90-93) as float[n][SRL_MAX_BODIES][8] = pos xyz, quat xyzw, mesh id;
 * n_bodies int32[n]; `Simulator.n_steps` (simulator.py:79-83) int32[n][2]; status bits int32[n]. */
int srl_get_state(srl_env* env, float* poses, int32_t* n_bodies, int32_t* substeps, int32_t* status);
/* `Observer.state` (observer.py:365-368) float[n][H*W], float[n][2^orientation_freedom][h*w]; `Rewarder` goal rect int32[n][4]. */
int srl_get_maps(srl_env* env, float* height, float* object_map, int32_t* goal_rect);
/* State injection for closed-form physics tests (host pointers, synchronises; either pointer may be NULL = leave as is):
 * `pb.resetBasePositionAndOrientation` (simulator.py:313) and `pb.resetBaseVelocity` (simulator.py:214) for every placed
 * body of every env, in the layouts srl_get_state / srl_get_velocities return (the mesh-id column is ignored). */
int srl_set_body_state(srl_env* env, const float* poses, const float* velocities);
/* `pb.stepSimulation` (simulator.py:219, :240, :320) x n_substeps on every env: no placement, no stop criterion, no
 * render — the raw sub-step the three loops of `Simulator.step` are built from. */
int srl_step_simulation(srl_env* env, int32_t n_substeps, void* stream);
/* solver telemetry int32[n]: sequential-impulse sweeps run by the last step of each env, all its sub-steps together
 * (each sub-step runs at most solver_iterations sweeps and ends them early on the residual threshold) */
int srl_get_sweeps(srl_env* env, int32_t* sweeps);
/* velocities float[n][SRL_MAX_BODIES][8] = lin xyz 0, ang xyz 0 */
int srl_get_velocities(srl_env* env, float* vel);
/* contact telemetry: deepest penetration (m) and number of manifold points per env */
int srl_get_contacts(srl_env* env, float* max_penetration, int32_t* n_points);

/* Renderer on explicit poses (test / profiling hook for the O1 row, observer.py:252-260):
 * poses_dev float[n][SRL_MAX_BODIES][7] (COM frame), mesh_ids_dev int32[n][SRL_MAX_BODIES],
 * n_bodies_dev int32[n] -> height_dev float[n][H*W]. */
int srl_render_heightmap(srl_env* env, const float* poses_dev, const int32_t* mesh_ids_dev,
                         const int32_t* n_bodies_dev, float* height_dev, void* stream);
/* O2 row: underside map(s) of one mesh (observer.py:262-277), host output float[2^orientation_freedom][h*w]. */
int srl_get_object_map(srl_env* env, int32_t mesh_id, float* object_map);

/* `StackEnv.render(mode='rgb_array')` (env.py:295-332; `TestStackEnv.render`, :558-596) of every env, on the device:
 * overhead_dev [n][H][W][3] = the overhead map coloured by elevation (R = m / max(m), or m where the max is 0; B = 1 - R, both
 * float32 values; G = 0.5, 0.5 + 0.1 inside the goal rectangle), object_dev [n][h][w][3] = the same of the object map on show
 * (orientation 0 of the pending rock; with ordering_freedom of the first rock still unplaced, `n[0]` of env.py:563; the empty
 * map when there is none; no goal).  The images are that function of exactly the arrays srl_get_maps returns.  Either
 * pointer may be NULL.  dtype 0: float64, the reference's return type; 1: uint8 frames, x * 255 + 0.5 in double, clamped to
 * 0 .. 255 and truncated.  Enqueued on `stream` like srl_step: it sees the maps of the steps before it there and does not
 * synchronise. */
int srl_render_rgb(srl_env* env, int32_t dtype, void* overhead_dev, void* object_dev, void* stream);

/* Perspective view of the pile itself, ray cast on the device (csrc/camera.hip): what `StackEnv(gui=True)` shows in
 * pybullet's viewer (simulator.py:140-146, env.py:275-281) — the rocks on the grey ground (simulator.py:167-179), a white
 * rectangle over the observable area and a green one over the goal (observer.py:423-426, rewarder.py:202-209). The definition,
 * float32 with one rounding per written operation unless said otherwise; fma(a, b, c) is the fused a * b + c, and
 * dot(a, b) = fma(a.x, b.x, fma(a.y, b.y, a.z * b.z)):
 *   scene    the rocks are the env's nb placed bodies (the pending rock at the spawn pose is not drawn); the ground is z = 0.
 *   camera   one for the whole call, handed over as finished vectors the host computes in double and rounds to float32: eye,
 *            fwd (unit), right and up (already scaled by tan(fov / 2) * W / H and tan(fov / 2)); no trigonometry on the device.
 *            Pixel (row i, column j) of the H x W image looks through its centre: s = float(2 j + 1) / float(W) - 1,
 *            u = 1 - float(2 i + 1) / float(H), d = (fwd + s * right) + u * up per component.  d is not normalised, so the ray
 *            parameter t is the depth along fwd, like a depth buffer's.
 *   rock     face f (unit normal n_f, offset d_f in the body's centre-of-mass frame) of a body at position x, rotation R
 *            (R from the quaternion as the solver makes it, row i of R . n = fma(R_i0, n.x, fma(R_i1, n.y, R_i2 * n.z))):
 *            nw = R . n_f, dw = d_f + dot(nw, x); for a ray from o along d: den = dot(nw, d), num = dw - dot(nw, o),
 *            t_f = num / den (the correctly rounded quotient).  t_in = max of t_f over the faces with den < 0 (the face
 *            of the lowest index among equals is "the face that gave t_in"), t_out = min of t_f over those with den > 0; a
 *            face with den == 0 and num < 0 makes the ray miss.  The ray from the eye hits the rock if t_in < t_out and
 *            t_in > 0.  The nearest hit is the smallest t_in over the bodies, the lowest slot among equals.
 *   ground   hit at t_g = -eye.z / d.z where d.z < 0; a rock wins where t_in < t_g.  A ray that hits neither is sky.
 *   shading  colour = albedo * (ambient + (diffuse * max(0, dot(n, light))) * lit) per channel; light is the unit vector
 *            towards the light.  Rock: albedo rock_rgb, n = nw of the face that gave t_in.  Ground: n = (0, 0, 1), albedo
 *            0.8 grey; where the hit point p = eye + t * d (fma(t, d, eye) per component) lies in the observable square
 *            [0, sx] x [0, sy], sx = sy = float(overhead_res) * pixel, the albedo is 0.5 * albedo + 0.5 (white), and where
 *            it also lies in the goal rectangle [float(u) * pixel, float(u + h) * pixel] x [float(v) * pixel,
 *            float(v + w) * pixel] (rewarder.py:205-206) that is blended again, 0.5 * albedo + 0.5 * (0, 1, 0).  lit = 1; with
 *            `shadows` lit = 0 where the ray from p + 1e-4 * n (fma per component) along light passes through any rock
 *            (t_in < t_out and t_out > 0, t_in = -inf and t_out = +inf before the first face).  Sky is sky_rgb.
 *   uint8    x * 255 + 0.5 in double, clamped to 0 .. 255, truncated (the rule of the overhead frames above).
 * Yaw and pitch are the host's business (stackrl_amd/camera.py); pybullet is on no machine of this project, so that
 * convention is this build's own and is not pinned to the viewer's.
 *
 * Scene: with the four scene pointers NULL the env's own state (poses, mesh ids, body count, goal); otherwise explicit, in
 * the layouts of the height-map hook above — poses_dev float[n][SRL_MAX_BODIES][7], mesh_ids_dev int32[n][SRL_MAX_BODIES],
 * n_bodies_dev int32[n] — plus goal_rect_dev int32[n][4] = (u, v, h, w): all four set or all four NULL.
 * Outputs, any of them NULL but not all: rgb_dev uint8[n][H][W][3]; depth_dev float[n][H][W], t of the hit, +inf for sky;
 * ids_dev int32[n][H][W], the body slot, -1 ground, -2 sky.  Enqueued on `stream` like a step: it sees the steps before it there,
 * does not synchronise, reads the env and writes only the outputs.  Refused with SRL_EINVAL: width or height outside
 * 1 .. 1024, a non-finite camera value, fwd or light not unit to 1e-3, a partial scene, all outputs NULL. */
typedef struct srl_camera {
  float eye[3], fwd[3], right[3], up[3], light[3], ambient, diffuse, rock_rgb[3], sky_rgb[3];
  int32_t width, height, shadows;
} srl_camera;
int srl_render_camera(srl_env* env, const srl_camera* cam, const float* poses_dev, const int32_t* mesh_ids_dev,
                      const int32_t* n_bodies_dev, const int32_t* goal_rect_dev, uint8_t* rgb_dev, float* depth_dev,
                      int32_t* ids_dev, void* stream);

/* ---- State records: save, restore and fork env states on the device (csrc/state.hip).
 * One env's persistent state is a record of 32-bit words, four parts in this order, each starting on a multiple of 4 words:
 * its header (episode machine, episode counter = RNG counter, goal, reward memory, episode list, script), the words of its
 * blob (poses, velocities, manifolds), its height map [overhead_res^2] and the staged render records of its rocks
 * [episode_length][stride][4].  The randomness is counter based (key = seed + env_index_offset + env index, counter = the
 * header's episode counter), so a record written back continues bit for bit; the key belongs to the SLOT: a record forked
 * into another env continues alike until that env's next reset, which draws the slot's own stream.  Not state: the
 * parameters, the mesh table, the error flags, timing, the launch order.
 *
 * Host arithmetic only, no handle, no device: the words of a record and the word offset of each of its four parts for a
 * configuration (n_envs and env_index_offset are not read).  Either output may be NULL. */
int srl_state_layout(const srl_config* cfg, int64_t* words, int64_t* part_offsets4);
/* What records must agree on to be written into this handle: the record layout, the size of the header, n_mesh and the
 * contents of the mesh table (hashed by srl_load_meshes), the configuration fields that shape the state or the kernels'
 * reading of it (episode_length, the resolutions, object_max_dimension, max_z, metric, goal_size_ratio, the reward scale and
 * exponents, place_at_com, the two freedoms, obs_dtype) and the source hash of srl_build_info.  n_envs and env_index_offset
 * are not part of it; the solver and physics parameters may differ between handles. */
int srl_state_signature(srl_env* env, uint64_t* signature);
/* Gathers the records of the envs idx_dev[0 .. n) (int32, device; NULL = all n = n_envs envs in order) into records_dev
 * [n][words] and returns the handle's seed and sample counter (host pointers, either may be NULL).  Enqueued on `stream`
 * like srl_step: no blocking copy, no allocation.  Refused with SRL_EINVAL while the staged records are stale: after
 * srl_load_meshes, srl_set_body_state, srl_kick or srl_step_simulation and before the next step. */
int srl_state_get(srl_env* env, const int32_t* idx_dev, int32_t n, void* records_dev, uint32_t* seed, uint32_t* sample_counter,
                  void* stream);
/* Env dst_idx_dev[i] takes record src_rec_dev[i] of records_dev, i < n (int32, device; NULL = i).  Records may repeat (a
 * fork); the destinations must be distinct and the record indexes inside the buffer (the caller's duty); an env index
 * outside the handle is skipped and reported by the next srl_sync_status.  A signature that is not the handle's own is
 * refused before any launch.  Enqueued on `stream`. */
int srl_state_set(srl_env* env, uint64_t signature, const int32_t* dst_idx_dev, const int32_t* src_rec_dev, int32_t n,
                  const void* records_dev, void* stream);
/* The handle's seed and sample counter, the episode counters left alone (srl_seed zeroes them): the rest of a full
 * restore.  A seed other than the handle's waits for the device first, like srl_seed. */
int srl_state_set_rng(srl_env* env, uint32_t seed, uint32_t sample_counter);

/* ---- Contact points: `Simulator.contact_points` (simulator.py:131-133, pybullet's getContactPoints; part of
 * `Simulator.state`, :135-138) of every env, gathered on the device (csrc/contacts.hip).  Nothing is simulated for it: the
 * manifolds and their accumulated impulses persist in every env's state between steps.  The definition, float32 with one
 * rounding per written operation; fma, dot as in the camera section, cross(a, b) = (fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x,
 * -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x))), R . v + x = per row i fma(R_i0, v.x, fma(R_i1, v.y, fma(R_i2, v.z, x_i))), R from
 * the body's quaternion as the solver makes it:
 *   order    of an env's contacts: first the ground points, body slot b ascending over b < nb, then point k < np ascending;
 *            then the pair points, manifold slot ascending over the slots in use, then point k ascending — the enumeration
 *            of srl_get_contacts, whose n_points is the count here.
 *   bodies   (a, b) as int32 body slots (the indexes of srl_get_state's poses), b = -1 for the ground.  pybullet's unique
 *            ids are not imitated: they depend on what else a client created (`draw_rectangle` bodies, the plane).
 *   row      srl_contact_row_words() = 20 float32 words: position on A xyz, position on B xyz (world coordinates), normal
 *            on B xyz (world, pointing from B towards A), distance (negative = penetration), normal force, lateral friction
 *            force 1 and its direction xyz, lateral friction force 2 and its direction xyz, and a word that is 0.
 *   ground   a = the body, b = -1.  Position on A = x + R . v, v = mesh vertex `vid` of the ground manifold in the body's
 *            centre-of-mass frame: the world vertex the settle kernel tests against the plane.  Position on B = that point
 *            dropped to the plane, (A.x, A.y, 0); the ground is the half-space z < 0.  Normal (0, 0, 1); the directions are the
 *            solver's, btPlaneSpace1 of +z: (0, -1, 0) and (1, -0, -0).  Distance = the manifold's (z of the vertex less the
 *            collision margin).
 *   pair     a manifold slot holds bodies i < j and, per point, la, lb, n, dist: la and lb are in the frames of i and j about
 *            their positions (the narrow phase stores R_i^T (p - x_i)), n is in world coordinates and points from j towards i
 *            (GJK's axis a - b; a positive normal impulse moves i along +n).  That is pybullet's convention with A = i, B = j,
 *            so a = i, b = j: neither swapped nor negated.  Position on A = x_i + R_i . la, on B = x_j + R_j . lb: the current
 *            pose applied to the manifold's local point, so after the sub-step's integration they are a sub-step newer than
 *            dist and n, which the narrow phase made before the solve (Bullet reports the positions of the narrow phase).
 *            The directions are btPlaneSpace1 of n as the solver evaluates it.
 *   forces   the accumulated impulse the manifold persists, divided (a correctly rounded quotient) by sim_time_step —
 *            pybullet's normalForce is the applied impulse over the time step: normal, direction 1, direction 2.  They are
 *            those of the last sub-step the step (or srl_step_simulation) ran.
 *   last_only  = 1 keeps the rows whose a or b is the last placed body, slot nb - 1, in their relative order:
 *            `Simulator.contact_points`.
 *   count    count_dev[e] is always the true total of the rows the call selects (all, or the last body's), whatever the
 *            capacity; only the first `capacity` of them are written, to bodies_dev [n][capacity][2] and rows_dev
 *            [n][capacity][20]; rows at or beyond min(count, capacity) are left untouched.
 *   wrench   optional, wrench_dev [n][episode_length][8] per body slot: net contact force xyz, number of its points, net
 *            contact torque about the body's position xyz, 0 (zeros for a slot >= nb).  Summed from zero over the body's rows
 *            in the order above, each sum one addition per component: a row gives its A the force F = fma(t2, f2, fma(t1, f1,
 *            n * fn)) per component and its B the force -F; the torque is cross(r, F) with r = the body's contact position
 *            less its position.  One lane per body, no atomics: a loop in that order gives the same bits.  It always covers
 *            all of the env's contacts, whatever capacity and last_only say.
 * Enqueued on `stream` like a step: it sees the steps before it there, does not synchronise, reads the env and writes only
 * the outputs (no header field, blob word or flag changes).  bodies_dev must be 8-byte aligned, rows_dev and wrench_dev
 * 16-byte.  Refused with SRL_EINVAL: a null env, a null count, bodies or rows pointer, capacity < 1, last_only outside
 * {0, 1}; with SRL_ENOMESH before srl_load_meshes. */
int32_t srl_contact_row_words(void);
/* The most points an env can hold: 4 * episode_length + 4 * manifold slots. */
int srl_contact_max_points(srl_env* env, int32_t* max_points);
int srl_contact_points(srl_env* env, int32_t last_only, int32_t capacity, int32_t* count_dev, int32_t* bodies_dev, float* rows_dev,
                       float* wrench_dev /* may be null */, void* stream);

/* ---- Push test: does the pile stand?  Fork it (the state records above), give its bodies a velocity increment, let it move
 * (srl_step_simulation), measure how far every body went — with no copy to the host (csrc/push.hip).  Three hooks: the poses
 * of every env (`Simulator.poses` / `positions`, simulator.py:85-93), the increment, and the distances
 * (`Simulator.distances`, simulator.py:95-111, and `distances_from_place`, :113-128).  In all three L = episode_length,
 * n = n_envs, nb = the env's number of placed bodies kept inside [0, L]; pose and velocity rows have the columns of
 * srl_get_state / srl_get_velocities with L slots per env in place of SRL_MAX_BODIES; every pointer is device memory, 16-byte
 * aligned (the body counts: 4); the call is enqueued on `stream` like a step, with no blocking copy and no allocation.
 * Float32 with one rounding per written operation; dot(a, b) = fma(a.x, b.x, fma(a.y, b.y, a.z * b.z)).
 *   poses      poses_dev [n][L][8]: x y z qx qy qz qw and the mesh id as the bit pattern of an int32, for the slots below nb;
 *              zero rows for the others.  n_bodies_dev [n] = nb.  The env is only read.
 *   kick       adds an increment to the velocities of the selected bodies, one float32 addition per component: the linear
 *              velocity takes columns 0 - 2 of the body's row of dv_dev, the angular one columns 4 - 6 (columns 3 and 7 are
 *              not read into anything).  per_body = 1: dv_dev is [n][L][8], a row per body slot; per_body = 0: dv_dev is
 *              [n][8], one row per env for every selected body.  select = SRL_KICK_ALL: every slot below nb; SRL_KICK_LAST:
 *              slot nb - 1, the last placed body; 0 .. L - 1: that slot where it is below nb.  A slot at or above nb is never
 *              written, so an env with nb = 0 is not touched.  Like srl_set_body_state it leaves the staged records stale:
 *              srl_state_get is refused until the next step.
 *   distances  per body slot b below nb a row of 4 words, rows_dev [n][L][4]: perr oerr dz speed (zeros for the others).  Its
 *              reference pose (p, a) is row b of ref_dev [n][L][8] — but the body's place pose, the one the reward's discount
 *              measures from, when ref_dev is NULL or b >= ref_nb_dev[e] (ref_nb_dev NULL: every row of ref_dev counts).  So
 *              with ref_dev = NULL the rows are `distances_from_place`, and with the poses and counts srl_poses gave before
 *              a step they are `Simulator.distances` of that step: a body new in it starts from its place pose
 *              (simulator.py:227-237).  With x, q the body's pose and v, w its velocities:
 *                perr  = sqrt(dot(d, d)), d = p - x per component
 *                oerr  = 2 acos(min(|(a0 q0 + a1 q1) + (a2 q2 + a3 q3)|, 1)), acos the library's own polynomial: what the
 *                        discounted metrics compute (rewarder.py:261-269)
 *                dz    = x.z - p.z
 *                speed = sqrt(dot(v, v))
 *   summary    summary_dev [n][8] per env: nb, moved, max perr, max oerr, the sum of perr, min dz, max speed, max
 *              sqrt(dot(w, w)) — all float32.  moved counts the bodies for which NOT (perr <= tol_p AND oerr <= tol_o), so a
 *              NaN counts as moved.  Every word is made by a loop over b = 0 .. nb - 1 in this order starting from 0: the
 *              maxima by fmax, the minimum by fmin (a NaN operand is passed over), the sum with one rounding per addition.
 *              No atomics: a loop in that order gives the same bits.
 * srl_poses and srl_pose_distances read the env and write only their outputs.  Refused with SRL_EINVAL before any launch: a
 * null env, a null output or increment pointer, a pointer off its alignment, per_body outside {0, 1}, select below
 * SRL_KICK_LAST or at or above L. */
#define SRL_KICK_ALL (-1)
#define SRL_KICK_LAST (-2)
int srl_poses(srl_env* env, float* poses_dev, int32_t* n_bodies_dev, void* stream);
int srl_kick(srl_env* env, const float* dv_dev, int32_t per_body, int32_t select, void* stream);
int srl_pose_distances(srl_env* env, const float* ref_dev /* may be null */, const int32_t* ref_nb_dev /* may be null */, float tol_p,
                       float tol_o, float* rows_dev, float* summary_dev, void* stream);

/* Per-kernel HIP-event timing (bench.py's roofline leg).  enable != 0 brackets every kernel launch of
 * srl_reset/srl_step with events on the launch stream; srl_get_kernel_times synchronises and returns the
 * accumulated milliseconds and launch counts since the last call: index 0 = settle (K1+K4),
 * 1 = render (K2+K5+obs pack), 2 = the staging kernel: the rocks' render records as a kernel of its own, for the explicit-pose hook and
 * for a step after a test hook moved bodies; in steady state the records are made in the settle kernel's tail, csrc/stage.h. */
int srl_set_profiling(srl_env* env, int32_t enable);

/* Tuning hint, between srl_create and srl_load_meshes: the number of envs that step on this device at the same time over
 * ALL handles of the caller (0 = this handle alone).  The reference's `ParallelEnv` has one process per env and a caller
 * is free to hold its batch as several handles (independent shards that step as their actions arrive, utils.py:468-486);
 * the settle kernel comes in a latency-oriented and a throughput-oriented build (9 - 16 rocks) and this number, not the
 * handle's own n_envs, says which one fits.  Results do not depend on it (the parity tests run both builds). */
int srl_set_concurrent_envs(srl_env* env, int32_t n_envs_on_device);

/* Test hook, after srl_load_meshes (which chooses it): the settle kernel variant this handle launches.  threads = threads
 * per env workgroup, points_per_thread = pair-manifold points per thread, kernel = 0: srl_k_step, up to 8 rocks; 1:
 * srl_k_step_pp1, 9 - 16 rocks, four waves; 2: srl_k_step_pp2, 17 - 32 rocks; 3: srl_k_step_t128, 9 - 16 rocks, two waves.
 * Any output may be null. */
int srl_get_step_variant(srl_env* env, int32_t* threads, int32_t* points_per_thread, int32_t* kernel);

/* Launch order of the settle kernel's workgroups (one per env).  The reference's `ParallelEnv` collects its worker
 * processes' results as they come (utils.py:540-543) and a vectorised step lasts as long as its slowest env (the stop
 * criterion of simulator.py:322-335); a batch that outnumbers the workgroups the device holds at once therefore starts the
 * envs with the longest expected settle first — those whose rock `Observer.pose` (observer.py:405-413) will release highest,
 * evaluated and sorted on the device before the step kernel.  mode -1 (default): by batch size (>= 2,048 envs), 0: index
 * order, 1: always ordered (at most 16,384 envs per handle).  Envs are independent: results do not depend on the order
 * (the parity tests run both). */
int srl_set_launch_order(srl_env* env, int32_t mode);
int srl_get_kernel_times(srl_env* env, float* ms3, int32_t* launches3);
/* the two kernels of an ordered launch (keys + sort), which run before the settle kernel and are not part of its time:
 * accumulated milliseconds and launches since the last call; call srl_get_kernel_times first. */
int srl_get_order_kernel_times(srl_env* env, float* ms, int32_t* launches);
/* Test hook: keys [n_envs] and permutation [n_envs] of the latest ordered launch (order[k] = the env workgroup k served,
 * ascending keys = highest release first).  Synchronises the device. */
int srl_get_launch_order(srl_env* env, unsigned long long* keys, int32_t* order);

/* Test hook: the staged rock records of the latest step (csrc/stage.h: the settle kernel's tail -> srl_k_render), host array
 * float[n_envs][episode_length][srl_stage_record_stride()][4]: per rock its pixel bounding box, up-facing planes, outline
 * sides and, per row of ray-cast items, the columns and the ranges of the two lists that row sweeps (layout: render.hip).
 * Synchronises the device. */
int srl_get_stage_records(srl_env* env, float* records, int64_t n_floats);
int32_t srl_stage_record_stride(void);

/* How this library was built: "SRL_BUILD_INFO<variant|hash>" — variant "vectorised+rewritten" (clang's SLP vectoriser on and
 * the pass of stackrl_amd/isa_fix.py over the compiled assembly) or "safe" (built in one go without the vectoriser), hash =
 * sha256 prefix of the sources and flags (stackrl_amd/build.py; bench.py prints both). */
const char* srl_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* STACKRL_HIP_H_ */
