// env_host_main.hip — stand-alone check of stackrl_amd/csrc/env_host.h on a CPU (tests/test_env_host.py builds it with the
// host code under -fsanitize=address,undefined and runs it).  No HIP runtime call: no device is opened.  Exits non-zero at
// the first mismatch and says which one.
//
// The closed forms hold to the stated ulp because every length, origin and mass below is a dyadic rational with few bits:
// the COM-frame subtraction, the AABB extents, mass / 12 and the sums of squares are then exact in float32, and the one
// rounding left is the final reciprocal (inertia) or square root (radius).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../stackrl_amd/csrc/env_host.h"

namespace {

#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      printf("MISMATCH %s:%d: %s: ", __FILE__, __LINE__, #cond);            \
      printf(__VA_ARGS__);                                                  \
      printf("\n");                                                         \
      exit(1);                                                              \
    }                                                                       \
  } while (0)

int ulps(float a, float b) {   // distance in float32 steps (both finite, same sign)
  int32_t x, y;
  memcpy(&x, &a, 4); memcpy(&y, &b, 4);
  return abs(x - y);
}

struct Solid {
  std::vector<float> verts;   // link frame, xyz
  std::vector<int32_t> tris;
  float mass, com[3];
};

struct Pool {   // the arrays srl_load_meshes takes
  std::vector<float> verts, mass_com;
  std::vector<int32_t> vert_off{0}, tris, tri_off{0};
  void add(const Solid& s) {
    verts.insert(verts.end(), s.verts.begin(), s.verts.end());
    tris.insert(tris.end(), s.tris.begin(), s.tris.end());
    vert_off.push_back((int32_t)(verts.size() / 3));
    tri_off.push_back((int32_t)(tris.size() / 3));
    mass_com.push_back(s.mass);
    for (int k = 0; k < 3; ++k) mass_com.push_back(s.com[k]);
  }
  int n() const { return (int)mass_com.size() / 4; }
  int build(MeshTable& T) const { return T.build(verts.data(), vert_off.data(), tris.data(), tri_off.data(), mass_com.data(), n()); }
};

// sides (a, b, c) from the corner `o`; vertex i = (i & 1, i >> 1 & 1, i >> 2); twelve outward counter-clockwise triangles
const float BOX[3] = {0.0625f, 0.09375f, 0.125f};
Solid box() {
  const float o[3] = {0.25f, -0.5f, 0.75f};
  Solid s;
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 3; ++k) s.verts.push_back(o[k] + ((i >> k) & 1 ? BOX[k] : 0.0f));
  const int quads[6][4] = {{1, 3, 7, 5}, {0, 4, 6, 2}, {2, 6, 7, 3}, {0, 1, 5, 4}, {4, 5, 7, 6}, {0, 2, 3, 1}};   // +x -x +y -y +z -z
  for (const auto& q : quads) for (int t : {q[0], q[1], q[2], q[0], q[2], q[3]}) s.tris.push_back(t);
  s.mass = 0.75f;   // mass / 12 = 2^-4
  const float off[3] = {1.0f / 256, -1.0f / 512, 1.0f / 128};   // the inertial origin: off the box's centre
  for (int k = 0; k < 3; ++k) s.com[k] = o[k] + 0.5f * BOX[k] + off[k];
  return s;
}

// regular tetrahedron: centre + TET_S (+-1, +-1, +-1) with an even number of minus signs
const float TET_S = 0.03125f;
Solid tetrahedron() {
  const float t[3] = {-0.125f, 0.375f, 0.5f}, sg[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
  Solid s;
  for (const auto& g : sg) for (int k = 0; k < 3; ++k) s.verts.push_back(t[k] + TET_S * g[k]);
  s.tris = {0, 1, 2, 0, 2, 3, 0, 3, 1, 1, 3, 2};
  s.mass = 1.5f;    // mass / 12 = 2^-3
  const float off[3] = {1.0f / 256, 1.0f / 512, -1.0f / 256};
  for (int k = 0; k < 3; ++k) s.com[k] = t[k] + off[k];
  return s;
}

// what every closed mesh must show: edges, planes through their vertices, radius, inverse mass
void check_mesh(const MeshTable& T, int m, const Solid& s, int want_edges, const char* name) {
  const MeshHdr& M = T.mh[m];
  const int nv = (int)s.verts.size() / 3, nt = (int)s.tris.size() / 3;
  CHECK(M.nv == nv && M.nt == nt && M.ne == want_edges, "%s: nv %d nt %d ne %d", name, M.nv, M.nt, M.ne);
  for (int e = 0; e < M.ne; ++e) {
    const uchar4 E = T.me[M.eo + e];
    CHECK(E.x < E.y && E.y < nv && E.z != E.w && E.z < nt && E.w < nt, "%s: edge %d = (%d %d | %d %d)", name, e, E.x, E.y, E.z, E.w);
    for (int f : {(int)E.z, (int)E.w}) {
      const uchar4 t = T.mt[M.to + f];
      const bool a = t.x == E.x || t.y == E.x || t.z == E.x, b = t.x == E.y || t.y == E.y || t.z == E.y;
      CHECK(a && b, "%s: edge %d (%d %d) is not in its face %d", name, e, E.x, E.y, f);
    }
  }
  double r = 0.0;
  for (int k = 0; k < nv; ++k) {
    const float4 v = T.mv[M.vo + k];
    const float vc[3] = {v.x, v.y, v.z};
    for (int c = 0; c < 3; ++c)   // COM frame: one float subtraction
      CHECK(vc[c] == s.verts[3 * k + c] - s.com[c], "%s: vertex %d component %d", name, k, c);
    const double d = sqrt((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z);
    if (d > r) r = d;
  }
  CHECK(ulps(M.radius, (float)r) <= 1, "%s: radius %.9g, largest vertex norm %.9g", name, M.radius, r);
  CHECK(M.inv_mass == 1.0f / s.mass, "%s: inv_mass %.9g", name, M.inv_mass);
  CHECK(M.cx == s.com[0] && M.cy == s.com[1] && M.cz == s.com[2], "%s: centre of mass", name);
  for (int f = 0; f < nt; ++f) {
    const float4 p = T.mp[M.to + f];
    const uchar4 t = T.mt[M.to + f];
    CHECK(t.x == s.tris[3 * f] && t.y == s.tris[3 * f + 1] && t.z == s.tris[3 * f + 2], "%s: triangle %d", name, f);
    CHECK(fabs(sqrt((double)p.x * p.x + (double)p.y * p.y + (double)p.z * p.z) - 1.0) <= 1e-6, "%s: plane %d is not unit", name, f);
    for (int k = 0; k < nv; ++k) {
      const float4 v = T.mv[M.vo + k];
      const double nd = (double)p.x * v.x + (double)p.y * v.y + (double)p.z * v.z - (double)p.w;
      const bool on = k == t.x || k == t.y || k == t.z;
      if (on) CHECK(fabs(nd) <= 1e-6, "%s: vertex %d is %.3g off the plane of its face %d", name, k, nd, f);
      else CHECK(nd <= 1e-6, "%s: vertex %d is %.3g outside face %d (normal not outward)", name, k, nd, f);
    }
  }
}

void check_inertia(const MeshHdr& M, float mass, double lx, double ly, double lz, const char* name) {
  const double want[3] = {12.0 / (mass * (ly * ly + lz * lz)), 12.0 / (mass * (lz * lz + lx * lx)), 12.0 / (mass * (lx * lx + ly * ly))};
  const float got[3] = {M.iix, M.iiy, M.iiz};
  for (int k = 0; k < 3; ++k)
    CHECK(ulps(got[k], (float)want[k]) <= 1, "%s: inverse inertia %d is %.9g, closed form %.9g", name, k, got[k], want[k]);
}

void test_mesh_table() {
  const Solid B = box(), Tt = tetrahedron();
  Pool both; both.add(B); both.add(Tt);
  MeshTable T;
  CHECK(both.build(T) == SRL_OK, "%s", g_err);
  CHECK(T.mh.size() == 2 && T.mv.size() == 12 && T.mt.size() == 16 && T.mp.size() == 16 && T.me.size() == 24, "table sizes");
  CHECK(T.mh[0].vo == 0 && T.mh[0].to == 0 && T.mh[0].eo == 0 && T.mh[1].vo == 8 && T.mh[1].to == 12 && T.mh[1].eo == 18, "offsets");
  CHECK(T.vs == 8, "vertex stride %d of an 8- and a 4-vertex mesh", T.vs);
  check_mesh(T, 0, B, 18, "box");
  check_mesh(T, 1, Tt, 6, "tetrahedron");
  check_inertia(T.mh[0], B.mass, BOX[0], BOX[1], BOX[2], "box");
  check_inertia(T.mh[1], Tt.mass, 2 * TET_S, 2 * TET_S, 2 * TET_S, "tetrahedron");
  int seen[6] = {0, 0, 0, 0, 0, 0};   // box normals: each of +-x, +-y, +-z exactly, twice
  for (int f = 0; f < 12; ++f) {
    const float4 p = T.mp[f];
    const float n[3] = {p.x, p.y, p.z};
    int axis = -1;
    for (int k = 0; k < 3; ++k) {
      if (fabsf(n[k]) == 1.0f) { CHECK(axis < 0, "box plane %d has two unit components", f); axis = k; }
      else CHECK(n[k] == 0.0f, "box plane %d: component %d is %.9g", f, k, n[k]);
    }
    CHECK(axis >= 0, "box plane %d has no axis", f);
    seen[2 * axis + (n[axis] < 0.0f)] += 1;
  }
  for (int k = 0; k < 6; ++k) CHECK(seen[k] == 2, "box normal %d appears %d times", k, seen[k]);

  Pool alone; alone.add(Tt);
  MeshTable T1, T2;
  CHECK(alone.build(T1) == SRL_OK && T1.vs == 4, "vertex stride %d of a 4-vertex mesh", T1.vs);
  CHECK(both.build(T2) == SRL_OK && T2.hash == T.hash && T1.hash != T.hash, "hash of equal / other inputs");
  Pool turned = both;   // the same surface, the first triangle's indices rotated
  const int32_t t0 = turned.tris[0];
  turned.tris[0] = turned.tris[1]; turned.tris[1] = turned.tris[2]; turned.tris[2] = t0;
  CHECK(turned.build(T2) == SRL_OK && T2.hash != T.hash, "hash after one changed triangle index");
}

void refused(const Pool& p, const char* text, const char* what) {
  MeshTable T;
  g_err[0] = 0;
  const int rc = p.build(T);
  CHECK(rc == SRL_EINVAL && !strcmp(g_err, text), "%s: rc %d, text '%s'", what, rc, g_err);
}

Solid padded(int nv, int nt) {   // a tetrahedron's arrays resized to the given counts (the count check comes before any index)
  Solid s = tetrahedron();
  s.verts.resize(3 * (size_t)nv, 0.0f);
  s.tris.resize(3 * (size_t)nt, 0);
  return s;
}

void test_refusals() {
  const char* counts = "mesh exceeds SRL_MAX_VERTS/SRL_MAX_TRIS";
  const char* open = "mesh is not a closed surface (an edge has only one face)";
  const Solid Tt = tetrahedron();
  { Pool p; p.add(padded(3, 4)); refused(p, counts, "3 vertices"); }
  { Pool p; p.add(padded(SRL_MAX_VERTS + 1, 4)); refused(p, counts, "too many vertices"); }
  { Pool p; p.add(padded(4, 3)); refused(p, counts, "3 triangles"); }
  { Pool p; p.add(padded(4, SRL_MAX_TRIS + 1)); refused(p, counts, "too many triangles"); }
  { Pool p; p.add(padded(SRL_MAX_VERTS, 4)); MeshTable T; CHECK(p.build(T) == SRL_OK && T.vs == SRL_MAX_VERTS, "SRL_MAX_VERTS vertices are admitted: %s", g_err); }
  for (int bad : {4, -1}) { Solid s = Tt; s.tris[7] = bad; Pool p; p.add(box()); p.add(s); refused(p, "triangle index out of range", "index"); }
  {   // three distinct vertices on one line
    Solid s = Tt;
    s.verts = {0, 0, 0, 0.25f, 0, 0, 0.5f, 0, 0, 0, 0.25f, 0};
    s.tris = {0, 1, 2, 0, 2, 3, 0, 3, 1, 1, 3, 2};
    Pool p; p.add(s); refused(p, "degenerate triangle", "zero-area triangle");
  }
  { Solid s = Tt; s.tris[4] = 0; Pool p; p.add(s); refused(p, "degenerate triangle", "a == b in an edge"); }   // (0, 0, 3)
  {   // a tetrahedron that has lost a face has three triangles, which the count check refuses first; the smallest open form it
    // admits: the face (1, 3, 2) split at its centroid (a closed surface of 5 vertices and 6 triangles), then (0, 1, 2) removed
    Solid s = Tt;
    s.tris.resize(9);
    { Pool p; p.add(s); refused(p, counts, "tetrahedron without a face, 3 triangles"); }
    s = Tt;
    for (int k = 0; k < 3; ++k) s.verts.push_back((s.verts[3 + k] + s.verts[9 + k] + s.verts[6 + k]) / 3.0f);
    s.tris = {0, 1, 2, 0, 2, 3, 0, 3, 1, 1, 3, 4, 3, 2, 4, 2, 1, 4};
    { Pool p; p.add(s); MeshTable T; CHECK(p.build(T) == SRL_OK && T.mh[0].ne == 9, "split tetrahedron: %s", g_err); }
    s.tris.erase(s.tris.begin(), s.tris.begin() + 3);
    { Pool p; p.add(s); refused(p, open, "tetrahedron without a face"); }
  }
  { Solid s = Tt; s.tris.insert(s.tris.end(), {0, 1, 2}); Pool p; p.add(s);
    refused(p, "mesh is not a closed two-manifold (an edge has more than two faces)", "duplicated face"); }
  { Pool p; p.add(Tt); p.vert_off[0] = -1; refused(p, "mesh offsets must not be negative", "negative vertex offset"); }
  { Pool p; p.add(Tt); p.tri_off[0] = -4; refused(p, "mesh offsets must not be negative", "negative triangle offset"); }
}

srl_config config(int L) {
  srl_config c;
  memset(&c, 0, sizeof c);
  c.n_envs = 1; c.episode_length = L; c.overhead_res = 128; c.object_res = 32;
  c.object_max_dimension = 0.125f; c.max_z = 0.375f; c.sim_time_step = 0.01f; c.goal_size_ratio = 0.25f; c.reward_scale = 1.0f;
  c.metric = SRL_METRIC_IOU; c.obs_dtype = SRL_DTYPE_UINT8;
  return c;
}

void test_layout() {
  size_t worst = 0; int worst_L = 0, worst_vs = 0;
  for (int conc : {0, 3072})
    for (int L = 1; L <= SRL_MAX_BODIES; ++L) {
      DevParams P0;
      CHECK(host_params(config(L), P0) == SRL_OK, "%s", g_err);
      const StepVariant v = step_variant_of(P0, conc);
      const StepVariant want = L <= 8 ? STEP_2W_PP1 : L > 16 ? STEP_4W_PP2 : conc >= 3072 ? STEP_2W_PP2 : STEP_4W_PP1;
      CHECK(v == want, "variant %d of %d rocks, %d envs at a time (want %d)", v, L, conc, want);
      CHECK(step_variant_of(P0, 3071) == (L > 8 && L <= 16 ? STEP_4W_PP1 : want), "variant of %d rocks below 3,072 envs", L);
      int prev = 0;
      for (int vs = 4; vs <= SRL_MAX_VERTS; ++vs) {
        DevParams P = P0;
        P.VS = vs;
        layout(P, conc);
        const int NS = P.NS, NP = P.NP;
        CHECK(NS == nslots(L) && NP == (L > 1 ? L * (L - 1) / 2 : 1), "slots %d pairs %d at %d rocks", NS, NP, L);
        const int off[] = {P.OFF_V, P.OFF_X, P.OFF_Q, P.OFF_PX, P.OFF_PQ, P.OFF_MESH, P.OFF_GM, P.OFF_MAN, P.OFF_SOP, P.OFF_POS, P.OFF_COL, P.BLOB};
        const int size[] = {8 * L, 4 * L, 4 * L, 4 * L, 4 * L, L, SRL_GM_WORDS * L, SRL_MAN_WORDS * NS, NP, NS, NS};
        CHECK(off[0] == 0 && P.OFF_W == 1, "velocities at %d / %d", P.OFF_V, P.OFF_W);
        for (int k = 0; k < 11; ++k) CHECK(off[k] + size[k] <= off[k + 1], "blob region %d [%d, +%d) reaches into %d (L %d)", k, off[k], size[k], off[k + 1], L);
        CHECK(P.BLOB % 4 == 0 && P.BLOB == P0.BLOB, "BLOB %d at stride %d, %d at 4 (L %d)", P.BLOB, vs, P0.BLOB, L);
        const bool lv = k_step_variants[v].lds_verts;
        CHECK((P.S_LV == -1) == !lv, "S_LV %d of variant %d", P.S_LV, v);
        const int s[] = {P.S_R, P.S_IW, P.S_AMIN, P.S_AMAX, P.S_BC, P.S_WV, lv ? P.S_LV : P.S_WV + 1, P.S_USED, P.S_MISC, P.S_PAIR, P.LDS_WORDS - P.BLOB};
        CHECK(s[0] == 0, "scratch starts at %d", s[0]);
        for (int k = 0; k < 10; ++k) CHECK(s[k] < s[k + 1], "scratch region %d at %d, the next at %d (L %d, stride %d)", k, s[k], s[k + 1], L, vs);
        CHECK(P.S_USED % 2 == 0 && P.S_PAIR + NP == P.LDS_WORDS - P.BLOB, "scratch tail (L %d, stride %d)", L, vs);
        CHECK(P.LDS_WORDS >= prev, "LDS_WORDS falls from %d to %d at stride %d (L %d)", prev, P.LDS_WORDS, vs, L);
        prev = P.LDS_WORDS;
        if (sizeof(float) * (size_t)P.LDS_WORDS > worst) { worst = sizeof(float) * (size_t)P.LDS_WORDS; worst_L = L; worst_vs = vs; }
      }
    }
  printf("largest admitted LDS size: %zu bytes at episode_length %d, vertex stride %d: the 160 KB refusal is %s\n", worst, worst_L,
         worst_vs, worst > 160 * 1024 ? "reachable" : "unreachable");
}

}  // namespace

int main() {
  test_mesh_table();
  test_refusals();
  test_layout();
  printf("env_host: ok\n");
  return 0;
}
