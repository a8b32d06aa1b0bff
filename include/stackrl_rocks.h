/* stackrl_rocks.h — C-ABI of libstackrl_rocks.so: the procedural rock generator on the device.
 *
 * The reference writes its rock pool with `stackrl/envs/data/generator.py` (`box`, :68-117, and `generate`, :124-266);
 * `stackrl_amd.assets.generate_rock` restates that on scipy, one rock at a time.  Here one wavefront makes one rock, from the
 * noise to the mass properties, and a batch of rocks is one launch.
 *
 * THE DEFINITION (stated here once; tests/rocks_cases.py restates it in numpy, float64 throughout):
 *
 *   1. Points.  P = 8 / 26 / 98 / 386 for 0..3 subdivisions.  Point k < 8 is the box corner
 *        (sx, sy, sz) * ext / 2,  sign bits of k = (x, y, z) from the high bit,  ext = extents * 2 radius / |extents|;
 *      point k >= 8 is the midpoint of its two parents, in the order `assets._subdivide` numbers them (the midpoint
 *      subdivision of the 12-triangle box has a fixed topology: a constant parent table).  A point of level l (0 for the
 *      corners, then 1..3) gets, per coordinate j, the noise
 *        scale_l * clip(ndtri(Fa + u * (Fb - Fa)), -1 / irregularity, 1 / irregularity),   scale_l = irregularity radius 2^-l,
 *        Fa = Phi(-1 / irregularity), Fb = 1 - Fa,   u = (x + 0.5) 2^-32,
 *        x = Philox4x32-10(counter = (g & 0xffffffff, g >> 32, 3 k + j, 0), key = (seed, 0x524f434b))[0],
 *      g = first_index + i the global rock index, so a rock does not depend on the batch it is made in.  Everything is
 *      float64 (midpoints of noisy parents included) and a point is rounded to float32 once, at the end.  The density is
 *      density_lo + u (density_hi - density_lo) with the draw of counter word 2 = 0xffffffff.
 *   2. Hull of the float32 points by gift wrapping: the start vertex is the lowest (x, y, z, index); the first edge comes
 *      from a pivot about the line through it along +y; faces are wrapped over a first-in first-out list of open directed
 *      edges.  A pivot about (a, b) is the point c that leaves every other point q with orient(a, b, c, q) <= 0,
 *        orient = ((b - a) x (c - a)) . (q - a),  float64 on the float32 points, one rounding per written operation,
 *      found by a tournament (ties: the lower index).  Vertices are numbered by ascending point index, triangles in the order
 *      the wrap emits them, (a, b, c) outward counter-clockwise.  A rock is ok (status 0) only if no directed edge came
 *      twice, every directed edge has its opposite, F = 2 V - 4 (Euler), and every point lies on or behind every face (exact
 *      ties between coplanar points can fold a wrap that still closes); more than SRL_MAX_VERTS vertices or SRL_MAX_TRIS
 *      faces is status 1 (overflow), everything else status 2 (degenerate).  Every loop is bounded by those limits.
 *   3. Centre of mass com by signed tetrahedra (float64).  Scale s = min(1, radius / max |p - com|) for fit 0 and
 *      min(1, 2 radius / longest box extent) for fit 1.
 *   4. The minimum-volume box over every (face normal, hull edge projected into the face's plane) pair; axes sorted by
 *      ascending extent, made right-handed, then turned by 90 degrees about Y (generator.py:207-210): the final extents are
 *      x >= y >= z.  xform = (s, R row-major, c): final = s R (point - c), the float32 values as stored.
 *   5. Volume, centre of mass, inertia and the metrics from the final float32 vertices, float64 accumulation.
 *
 * Sums and extrema have a fixed order (a lane's elements ascending, then a butterfly over the wave): the same inputs give the
 * same bits.  A rock whose status is not 0 has counts (0, 0) and zeros elsewhere; its points_out are written.
 *
 * Plain C, device pointers owned by the caller, contiguous, `stream` is a hipStream_t as void*; returns 0 on success.
 */
#ifndef STACKRL_ROCKS_H_
#define STACKRL_ROCKS_H_

#include <stdint.h>

#include "srl_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRL_ROCKS_MAX_POINTS 386
#define SRL_ROCKS_OK 0
#define SRL_ROCKS_OVERFLOW 1
#define SRL_ROCKS_DEGENERATE 2

typedef struct srl_rocks_params {
  float radius;          /* 0.0625 */
  float irregularity;    /* (0, 1] */
  float extents[3];      /* (1, 1/2, 1/3): ratios, scaled to the sphere of `radius` as generator.py:85-86 */
  int32_t subdivisions;  /* 0..3 -> 8 / 26 / 98 / 386 points */
  float density_lo, density_hi;   /* 2200, 2600 */
  int32_t fit;           /* 0: bounding sphere about the centre of mass (what assets.box_rock does and the shipped pool has);
                            1: 2*radius / longest OBB extent (generator.py:114-116) */
  uint32_t seed;
} srl_rocks_params;

/* The number of points of a rock of `subdivisions` (0..3); another value returns 1 (SRL_EINVAL). */
int srl_rocks_points(int32_t subdivisions, int32_t* n_points);

/* Rocks first_index .. first_index + n - 1.  Enqueues on `stream`, allocates nothing, returns.  Returns 1 (SRL_EINVAL), with a
 * text of its own behind srl_rocks_last_error, for: irregularity outside (0, 1] when points_in_dev is NULL; subdivisions
 * outside 0..3; n < 1; a null required pointer (p and every output but points_out_dev); with points_in_dev, n_points_in
 * outside 4..386; a radius, extents or fit that make no box.  A launch error returns 4. */
int srl_rocks_generate(const srl_rocks_params* p, int64_t first_index, int32_t n,
                       const float* points_in_dev,   /* NULL, or [n][P][3]: skip the noise stage, any P in 4..386 given by n_points_in */
                       int32_t n_points_in,
                       float* points_out_dev,        /* NULL, or [n][P][3]: the points the hull was taken of */
                       float* verts_dev,             /* [n][SRL_MAX_VERTS][3] */
                       int32_t* vert_src_dev,        /* [n][SRL_MAX_VERTS]: which input point each vertex is (-1 beyond nv) */
                       int32_t* tris_dev,            /* [n][SRL_MAX_TRIS][3], local, outward CCW */
                       int32_t* counts_dev,          /* [n][2] = nv, nt */
                       float* mass_com_dev,          /* [n][4], as srl_load_meshes takes it */
                       float* inertia_dev,           /* [n][6] ixx ixy ixz iyy iyz izz about the centre of mass, density applied */
                       float* xform_dev,             /* [n][13]: s, R (row-major), c  with  final = s * R * (point - c) */
                       float* metrics_dev,           /* [n][4]: volume, rectangularity, aspect ratio, OBB volume (generator.py:233-240's log) */
                       int32_t* status_dev,          /* [n]: 0 ok, 1 overflow (> SRL_MAX_VERTS / SRL_MAX_TRIS), 2 degenerate */
                       void* stream);

const char* srl_rocks_last_error(void);
const char* srl_rocks_build_info(void);

#ifdef __cplusplus
}
#endif
#endif  /* STACKRL_ROCKS_H_ */
