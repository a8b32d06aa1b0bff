// solver.h — the settle kernels' sequential-impulse solver (included by settle.hip, after Lds and the velocity load / store pair).
// The rows, two formulations of a sweep's ground phase and two of a colour's pair phase, and the sweep:
//   ground  GPoint / ground_turn (lane = ground point, turns through LDS), GBody / ground_body (lane = body, rows from LDS records)
//   pairs   Point / point_turn (lane = contact point), PSplit / pair_phase (two lanes = contact point, one per body)
// A kernel variant runs one of each (the booleans of Variant<T, PP>, settle.hip); stage (6) of substep makes their state and
// solver_sweep runs them.  (As policy structs behind one interface per phase the 8-rock kernel compiled to a slower register
// allocation, 2 - 3 % per launch: profiles/settle_solver_refactor_ab.txt.)
// ------------------------------------------------------------------ rows
// One solver row in precomputed form: direction d, ca = ra x d, aa = Ia ca (and cb, ab for body B),
// k = effective mass denominator.  Same expression trees as the sequential definition.
struct Row { v3 d, ca, aa, cb, ab; float rk, k; };   // k = effective mass denominator, rk = 1 / k

template <bool HAS_B>
__device__ __forceinline__ Row make_row(v3 d, v3 ra, v3 rb, float ima, const m3& Ia, float imb, const m3& Ib) {
  Row r;
  r.d = d;
  r.ca = cross(ra, d);
  r.aa = mmul(Ia, r.ca);
  r.cb = V(0.0f, 0.0f, 0.0f); r.ab = V(0.0f, 0.0f, 0.0f);
  float k = ima + dot(cross(r.aa, ra), d);
  if (HAS_B) {
    r.cb = cross(rb, d);
    r.ab = mmul(Ib, r.cb);
    k = k + (imb + dot(cross(r.ab, rb), d));
  }
  r.rk = 1.0f / k;
  r.k = k;
  return r;
}

// The pair rows in PAIR form (round 5).  A body's velocities leave LDS as the register pairs (v.c, w.c) (Lds::VW); a row's
// constants are kept as the matching pairs — ka[c] = (d.c, ca.c), ua[c] = (d.c ima, aa.c) for body A, kb[c] = (d.c, cb.c),
// ub[c] = (d.c (-imb), -ab.c) for body B — so that both dot products of a body are one chain of three packed operations, the
// velocity update of a body three packed FMAs, and no register move stands between a read, the rows and the write-back.  (The
// compiler's own pairing of row_solve — (va.c, vb.c), (wa.c, wb.c) across the two bodies — cost 23 moves and two sign flips per
// turn of 89 vector instructions.)  The operations and their order are row_solve's: fma(-ab.c, dl, wb.c) = fma(ab.c, -dl, wb.c)
// exactly (the product's sign is exact), the halves of a packed FMA round once each: bit-identical.
// (srl_k_step no longer runs these: it solves a pair contact on two lanes, HRow / pair_phase below; the other three variants do.)
struct PRow { f2 ka[3], kb[3], ua[3], ub[3]; float rk, k; };
struct Vel2 { f2 a[3], b[3]; };   // [c] = (v.c, w.c) of body A / B

__device__ __forceinline__ PRow pack_row(const Row& r, float ima, float imb) {
  PRow q;
  const v3 da = r.d * ima, db = r.d * (-imb);
  q.ka[0] = F2(r.d.x, r.ca.x); q.ka[1] = F2(r.d.y, r.ca.y); q.ka[2] = F2(r.d.z, r.ca.z);
  q.kb[0] = F2(r.d.x, r.cb.x); q.kb[1] = F2(r.d.y, r.cb.y); q.kb[2] = F2(r.d.z, r.cb.z);
  q.ua[0] = F2(da.x, r.aa.x); q.ua[1] = F2(da.y, r.aa.y); q.ua[2] = F2(da.z, r.aa.z);
  q.ub[0] = F2(db.x, -r.ab.x); q.ub[1] = F2(db.y, -r.ab.y); q.ub[2] = F2(db.z, -r.ab.z);
  q.rk = r.rk; q.k = r.k;
  return q;
}

__device__ __forceinline__ void prow_apply(const PRow& r, Vel2& u, float imp) {
  const f2 d2 = F2(imp, imp);
#pragma unroll
  for (int c = 0; c < 3; ++c) { u.a[c] = fma2(r.ua[c], d2, u.a[c]); u.b[c] = fma2(r.ub[c], d2, u.b[c]); }
}
// FRICTION: the row's target is 0 and r.rk holds -1 / k (make_pair_point): dl is the plain product vrel (-rk), which is
// fma(-vrel, rk, 0 rk) but for the sign of a zero that acc + dl does not see (the argument: GRow below)
template <bool FRICTION>
__device__ __forceinline__ void prow_solve(const PRow& r, Vel2& u, float target, float& acc, float lo, float hi, float& res) {
  const f2 sa = fma2(r.ka[0], u.a[0], fma2(r.ka[1], u.a[1], r.ka[2] * u.a[2]));   // (dot(d, va), dot(ca, wa))
  const f2 sb = fma2(r.kb[0], u.b[0], fma2(r.kb[1], u.b[1], r.kb[2] * u.b[2]));   // (dot(d, vb), dot(cb, wb))
  float ra = sa.x + sa.y;
  asm("" : "+v"(ra));   // (kept from the vectoriser: paired with the sum below the two adds cost three moves and a packed add)
  const float vrel = ra - (sb.x + sb.y);
  // (target - vrel) rk as one fused step and the linear impulses as (d m^-1) dl: the products that do not depend on the
  // velocities leave the dependency chain (10 dependent operations per row instead of 12; the oracle evaluates the same)
  float dl = FRICTION ? vrel * r.rk : fmaf(-vrel, r.rk, target * r.rk);
  // the accumulated impulse clamped to [lo, hi] as the median of the three (v_med3_f32; the oracle restates its zero
  // handling): one instruction on the solver's dependency chain instead of two compare / select pairs through VCC,
  // each of which costs a lone wave its wait states — 6.68 -> 6.02 ms per launch at the headline shape
  const float na = __builtin_amdgcn_fmed3f(acc + dl, lo, hi);
  dl = na - acc;
  acc = na;
  // res: running maximum of the rows' residuals |delta impulse x k| (Bullet: deltaImpulse / m_jacDiagABInv) — off the
  // velocities' dependency chain
  res = fmaxf(res, fabsf(dl * r.k));
  prow_apply(r, u, dl);
}

__device__ __forceinline__ float contact_target(const DevParams& P, float dist) {
  float inv_dt = 1.0f / P.c.sim_time_step;
  float pen = dist + P.c.linear_slop;   // Bullet: penetration = distance + m_linearSlop
  return pen > 0.0f ? -(pen * inv_dt) : -((pen * P.c.erp) * inv_dt);
}

// A contact point owned by one lane for the duration of a sub-step's solve
struct Point {
  PRow n, t1, t2;
  float target, in, i1, i2, ima, imb, mu;
  int a, b;        // bodies (b < 0: ground)
  int colour;      // -1 = ground phase
  int idx;         // position inside its manifold (turn order)
  bool valid;
};

// Ground rows.  The ground's normal is +z and its tangents (plane_space of +z) are -y and +x: a ground row's direction is
// sgn e_axis, so its relative velocity takes one component of the linear velocity and its impulse changes that component
// only (stated so in the oracle too): 13 instead of 25 operations per row, and 8 instead of 17 registers of row constants.
//
// The rows' structural zeros.  ca = ra x d is perpendicular to d = sgn e_axis, so its component `axis` is an exact zero in every
// ground row, and the other six components of a point's three rows are four values:
//   normal    (+z)  ca = ( ra.y, -ra.x,   ±0 )
//   tangent 1 (-y)  ca = ( ra.z,   ±0, -ra.x )
//   tangent 2 (+x)  ca = (  ±0,  ra.z, -ra.y )
// (cross() of ra with (0, 0, 1), (0, -1, 0), (1, -0, -0): every other product in it has a zero factor.)  The rows are solved
// from c[0] = n.ca.x, c[1] = n.ca.y (for t1.ca.z), c[2] = t1.ca.x (for t2.ca.y), c[3] = t2.ca.z — the values cross() gave,
// not a restatement from ra — and the oracle's chain fma(ca.x, w.x, fma(ca.y, w.y, fma(ca.z, w.z, sgn v[axis]))) is evaluated
// without the term of component `axis`, the others in their places.  The set-up (aa = Ia ca, k) is the general row's, in full.
// Why every stored value stays what the oracle computes (finite velocities; a diverged env is outside the claim):
//   - fma(±0, w, s) is s for finite w unless s is itself a zero, and then it is a zero: leaving the term out can change the
//     sign of an exactly zero vrel and nothing else.  A shared word differs from the one it stands for only where a
//     component of ra is an exact zero, and then as a zero of the other sign: the same case.
//   - dl = fma(-vrel, rk, target rk) is target rk whatever the sign of a zero vrel, unless target rk is a zero.  The friction
//     rows' target is 0 and their dl is formed as the plain product vrel (-rk) (their records hold -rk: one v_mul_f32 in its
//     32-bit encoding instead of an FMA with the product 0 rk for an addend): it is fma(-vrel, rk, +0) bit for bit unless it is
//     a zero, where it can be -0 for the oracle's +0.  The normal row keeps target rk, which is -0 when dist + linear_slop
//     is 0: there too dl can only be a zero of the other sign.
//   - acc + dl with dl a zero of either sign is acc, including acc = +0; and acc is never -0: the impulses start from +0
//     (a new contact) or from acc warmstart, and the clamp med3(acc + dl, lo, hi) returns a -0 only for acc + dl = -0 (which
//     takes acc = dl = -0) or for a bound -0 that wins, which it cannot: the normal row's lo is +0 and a friction row's
//     bounds are ∓lim with lim = mu acc_n >= +0, where med3 orders -0 below +0 and returns +0 for lim = +0 (oracle: med3f).
//     (A warmstart factor of 0 would make a -0 of a negative friction impulse; the next acc is then still the oracle's by
//     value.)  The impulse applied to the velocities is na - acc, formed after the clamp from equal values: every velocity
//     update sees the oracle's bits.
struct GRow { v3 aa; float rk, k; };      // (n: rk = 1 / k; t1, t2: see GPoint)
struct GPoint {
  GRow n, t1, t2;                          // t1.rk, t2.rk = -1 / k: a friction row's dl is vrel (-rk)
  float c[4];                              // the rows' non-zero ca components (above)
  float target, in, i1, i2, ima;
  int a, idx;
  bool valid;
};

// the ground points' friction coefficient: one value for all of them, so no point or record carries it
__device__ __forceinline__ float ground_mu(const srl_config& c) { return c.friction_rock * c.friction_ground; }

__device__ __forceinline__ GRow make_grow(v3 d, v3 ra, float ima, const m3& Ia, v3& ca) {
  GRow r;
  ca = cross(ra, d);
  r.aa = mmul(Ia, ca);
  const float k = ima + dot(cross(r.aa, ra), d);
  r.rk = 1.0f / k;
  r.k = k;
  return r;
}

template <int AXIS, int SGN>
__device__ __forceinline__ void grow_apply(v3 aa, float ima, v3& v, v3& w, float imp) {   // aa: the row's GRow::aa
  float& va = AXIS == 0 ? v.x : AXIS == 1 ? v.y : v.z;
  va = fmaf(SGN < 0 ? -ima : ima, imp, va);
  w = madd(w, aa, imp);
}
// a ground row solved, from its constants — c0, c1: the components of ca other than AXIS, in x, y, z order — and, for the normal
// row, the product trk = target * rk (off the velocities' chain: the body lanes read it from their records, cg_store).  The
// friction rows (AXIS != 2) are called with rk = -1 / k; their trk is not read.
template <int AXIS, int SGN>
__device__ __forceinline__ void grow_solve_t(float c0, float c1, v3 aa, float rk, float k, float ima, v3& v, v3& w, float trk,
                                             float& acc, float lo, float hi, float& res) {
  float& va = AXIS == 0 ? v.x : AXIS == 1 ? v.y : v.z;
  const float w0 = AXIS == 0 ? w.y : w.x, w1 = AXIS == 2 ? w.y : w.z;
  const float vrel = fmaf(c0, w0, fmaf(c1, w1, SGN < 0 ? -va : va));
  float dl = AXIS != 2 ? vrel * rk : fmaf(-vrel, rk, trk);
  const float na = __builtin_amdgcn_fmed3f(acc + dl, lo, hi);
  dl = na - acc;
  acc = na;
  res = fmaxf(res, fabsf(dl * k));
  grow_apply<AXIS, SGN>(aa, ima, v, w, dl);
}
template <int AXIS, int SGN>
__device__ __forceinline__ void grow_solve(float c0, float c1, const GRow& r, float ima, v3& v, v3& w, float target, float& acc,
                                           float lo, float hi, float& res) {
  grow_solve_t<AXIS, SGN>(c0, c1, r.aa, r.rk, r.k, ima, v, w, target * r.rk, acc, lo, hi, res);
}

__device__ __forceinline__ GPoint make_ground_point(const Lds& L, int b, int i) {
  const DevParams& P = *L.P;
  GPoint p;
  p.valid = false; p.a = b; p.idx = i;
  p.in = 0.0f; p.i1 = 0.0f; p.i2 = 0.0f; p.target = 0.0f; p.ima = 0.0f;
  const float* g = L.GM(b);
  if (i >= __float_as_int(g[0])) return p;
  p.valid = true;
  p.ima = L.BC(b)[0];
  const m3 Ia = ldm(L.IW(b));
  const int vid = __float_as_int(g[SRL_GM_VID + i]);
  const v3 pw = ld3(L.WV(b) + 3 * vid);
  const v3 ra = V(pw.x, pw.y, pw.z - P.c.collision_margin) - ld3(L.X(b));
  v3 n = V(0.0f, 0.0f, 1.0f), t1, t2;
  plane_space(n, t1, t2);   // (0, -1, 0), (1, -0, -0)
  v3 cn, c1, c2;
  p.n = make_grow(n, ra, p.ima, Ia, cn);
  p.t1 = make_grow(t1, ra, p.ima, Ia, c1);
  p.t2 = make_grow(t2, ra, p.ima, Ia, c2);
  p.c[0] = cn.x; p.c[1] = cn.y; p.c[2] = c1.x; p.c[3] = c2.z;
  p.t1.rk = -p.t1.rk; p.t2.rk = -p.t2.rk;
  p.target = contact_target(P, g[SRL_GM_DIST + i]);
  p.in = g[SRL_GM_IN + i]; p.i1 = g[SRL_GM_T1 + i]; p.i2 = g[SRL_GM_T2 + i];
  return p;
}

// one turn of a ground point: the body's velocities, three axis rows, write back
template <bool WARM>
__device__ __forceinline__ void ground_turn(const Lds& L, GPoint& p, float mu, float& res) {
  const float ws = L.P->c.warmstart;
  v3 v, w;
  vw_load(L.VW(p.a), v, w);
  if (WARM) {
    p.in = p.in * ws; p.i1 = p.i1 * ws; p.i2 = p.i2 * ws;
    grow_apply<2, 1>(p.n.aa, p.ima, v, w, p.in);
    grow_apply<1, -1>(p.t1.aa, p.ima, v, w, p.i1);
    grow_apply<0, 1>(p.t2.aa, p.ima, v, w, p.i2);
  } else {
    grow_solve<2, 1>(p.c[0], p.c[1], p.n, p.ima, v, w, p.target, p.in, 0.0f, 1e30f, res);
    const float lim = mu * p.in;
    grow_solve<1, -1>(p.c[2], p.c[1], p.t1, p.ima, v, w, 0.0f, p.i1, -lim, lim, res);
    grow_solve<0, 1>(p.c[2], p.c[3], p.t2, p.ima, v, w, 0.0f, p.i2, -lim, lim, res);
  }
  vw_store(L.VW(p.a), v, w);
}

// ---- the ground phase by BODY lanes (round 5).  The (up to 4) ground points of one body share that body's velocities and
// nothing else, so a sweep's ground phase is, per body, a sequence of 4 x 3 rows on one pair (v, w).  As turns of point lanes
// the pair went through LDS between the points (write, read, wait: ~100 cycles a turn, and a lone wave has nothing to hide
// them under); here lane = body keeps (v, w) and the points' accumulated impulses in registers for the whole phase and reads
// the rows' constants — made once per sub-step by the point lanes, as before — from LDS in the order it consumes them
// (reads that depend on nothing the rows compute).  Same rows, same order per body, same expression trees: bit-identical.
#define SRL_CG_WORDS 20      // per ground point: 5 float4 (layout: cg_store)
struct GBody {
  float acc[SRL_GMAXP][3];   // accumulated impulses (normal, tangent 1, tangent 2) of the body's ground points
  float ima;
  int np, b;                 // points in the body's ground manifold (0: none / not a body lane)
  float* pvw;                // the body's velocities in LDS (Lds::VW)
  const float4* rec;         // its points' row constants
};

__device__ __forceinline__ float4* cg_rec(const Lds& L, int b, int i) {   // aliases the world vertices, dead during the solve
  return (float4*)L.WV(0) + (SRL_CG_WORDS / 4) * (SRL_GMAXP * b + i);
}
// A record holds what the rows read and nothing else, in the order ground_point consumes it: the four ca values (GRow: no
// zero words), aa, rk and k of each row (-1 / k for the friction rows) and the normal row's target rk.  No friction target (it is
// 0, and its product with rk is not formed) and no mu (ground_mu: a uniform value).  20 words against 28: five reads a point
// instead of seven, and in srl_k_step's sweeps 37 - 38 vector instructions a point instead of 40 - 41 (the fourth: 41 for 44).
// Measured with the friction product: +1.8 % env steps/s in the 20-step window, +1.1 - 3.0 % over six episodes; the shorter
// rows and records without it were no gain by the project's rule (profiles/ground_zero_terms_ab.txt).
__device__ __forceinline__ void cg_store(const Lds& L, const GPoint& p) {
  float4* r = cg_rec(L, p.a, p.idx);
  r[0] = make_float4(p.c[0], p.c[1], p.n.rk, p.target * p.n.rk);
  r[1] = make_float4(p.n.aa.x, p.n.aa.y, p.n.aa.z, p.n.k);
  r[2] = make_float4(p.c[2], p.c[3], p.t1.rk, p.t2.rk);
  r[3] = make_float4(p.t1.aa.x, p.t1.aa.y, p.t1.aa.z, p.t1.k);
  r[4] = make_float4(p.t2.aa.x, p.t2.aa.y, p.t2.aa.z, p.t2.k);
}

struct GRec { f4 q[5]; };   // one ground point's row constants (cg_store)

template <bool WARM>
__device__ __forceinline__ void ground_point(const GRec& R, GBody& gb, int i, float ws, float mu, v3& v, v3& w, float& res) {
  const f4 q0 = R.q[0], q1 = R.q[1], q2 = R.q[2], q3 = R.q[3], q4 = R.q[4];
  if (WARM) {
    gb.acc[i][0] = gb.acc[i][0] * ws; gb.acc[i][1] = gb.acc[i][1] * ws; gb.acc[i][2] = gb.acc[i][2] * ws;
    grow_apply<2, 1>(V(q1.x, q1.y, q1.z), gb.ima, v, w, gb.acc[i][0]);
    grow_apply<1, -1>(V(q3.x, q3.y, q3.z), gb.ima, v, w, gb.acc[i][1]);
    grow_apply<0, 1>(V(q4.x, q4.y, q4.z), gb.ima, v, w, gb.acc[i][2]);
  } else {
    grow_solve_t<2, 1>(q0.x, q0.y, V(q1.x, q1.y, q1.z), q0.z, q1.w, gb.ima, v, w, q0.w, gb.acc[i][0], 0.0f, 1e30f, res);
    const float lim = mu * gb.acc[i][0];
    grow_solve_t<1, -1>(q2.x, q0.y, V(q3.x, q3.y, q3.z), q2.z, q3.w, gb.ima, v, w, 0.0f, gb.acc[i][1], -lim, lim, res);
    grow_solve_t<0, 1>(q2.x, q2.y, V(q4.x, q4.y, q4.z), q2.w, q4.w, gb.ima, v, w, 0.0f, gb.acc[i][2], -lim, lim, res);
  }
}

__device__ __forceinline__ GRec cg_load(const float4* rec, int i) {
  GRec R;
#pragma unroll
  for (int k = 0; k < 5; ++k) { const float4 t = rec[5 * i + k]; R.q[k].x = t.x; R.q[k].y = t.y; R.q[k].z = t.z; R.q[k].w = t.w; }
  return R;
}

// ---- the record of point i + 1 requested while point i is computed (AHEAD).  A plain read whose only use sits in the guarded
// block of the next point is sunk into that block by the compiler (at IR level), a volatile one becomes a flat load with a
// wait behind it, an empty asm that pins the value waits for it: so the reads and their waits are written out.  cg_request
// issues the five 16-byte reads of record I (and passes `tie`, an operand the current point's first operation needs, through,
// so that the reads stand before that point's arithmetic); cg_arrive waits for everything in flight and passes the record and
// `tie` (a result of the current point's last row) through, so that the wait stands behind that arithmetic and the next point's
// in front of nothing it needs.  Every read is waited for in the block that issued it: no register is handed back to the
// allocator with a read still in flight.  (The compiler's own wait counts do not know these reads; they can only wait longer.)
template <int I>
__device__ __forceinline__ void cg_request(unsigned a, GRec& R, float& tie) {
  asm volatile(
      "ds_read_b128 %0, %6 offset:%7\n\tds_read_b128 %1, %6 offset:%8\n\tds_read_b128 %2, %6 offset:%9\n\t"
      "ds_read_b128 %3, %6 offset:%10\n\tds_read_b128 %4, %6 offset:%11"
      : "=&v"(R.q[0]), "=&v"(R.q[1]), "=&v"(R.q[2]), "=&v"(R.q[3]), "=&v"(R.q[4]), "+v"(tie)
      : "v"(a), "n"(80 * I), "n"(80 * I + 16), "n"(80 * I + 32), "n"(80 * I + 48), "n"(80 * I + 64));
}
// the body's (v, w) and record 0 in one go (the compiler's own read of (v, w) would be waited for with a count that does not
// know the records behind it: everything)
__device__ __forceinline__ void cg_request_first(unsigned avw, unsigned a, f4& a0, f2& a1, GRec& R) {
  asm volatile(
      "ds_read_b128 %0, %7\n\tds_read_b64 %1, %7 offset:16\n\t"
      "ds_read_b128 %2, %8\n\tds_read_b128 %3, %8 offset:16\n\tds_read_b128 %4, %8 offset:32\n\t"
      "ds_read_b128 %5, %8 offset:48\n\tds_read_b128 %6, %8 offset:64"
      : "=&v"(a0), "=&v"(a1), "=&v"(R.q[0]), "=&v"(R.q[1]), "=&v"(R.q[2]), "=&v"(R.q[3]), "=&v"(R.q[4])
      : "v"(avw), "v"(a));
}
__device__ __forceinline__ void cg_arrive_first(f4& a0, f2& a1, GRec& R) {   // the next record's five reads stay in flight
  asm volatile("s_waitcnt lgkmcnt(5)"
               : "+v"(a0), "+v"(a1), "+v"(R.q[0]), "+v"(R.q[1]), "+v"(R.q[2]), "+v"(R.q[3]), "+v"(R.q[4]));
}
template <int LEFT>   // LEFT: reads that may stay in flight (the record requested after this one)
__device__ __forceinline__ void cg_arrive(GRec& R, float& tie) {
  asm volatile("s_waitcnt lgkmcnt(%6)"
               : "+v"(R.q[0]), "+v"(R.q[1]), "+v"(R.q[2]), "+v"(R.q[3]), "+v"(R.q[4]), "+v"(tie)
               : "n"(LEFT));
}

// The ground phase of one body lane: its points in order on (v, w).  Without KEEP the pair is read from LDS here (AHEAD: in one go
// with record 0) and written back, and the caller's v, w are scratch.  KEEP: it stays in the caller's registers from sweep to
// sweep — sub-steps whose wave holds no pair point (half of all sub-steps, 20 - 85 % of the slowest envs') run their sweeps as the
// ground phase alone, and nothing else reads or writes the velocities during the solve.
template <bool WARM, bool AHEAD, bool KEEP>
__device__ __forceinline__ void ground_body(GBody& gb, float ws, float mu, v3& v, v3& w, float& res) {
  static_assert(SRL_CG_WORDS == 20, "cg_request reads five float4 per record");
  const float4* rec = gb.rec;
  // The guards are nested: the points of a manifold are a prefix.
  static_assert(SRL_GMAXP == 4, "four nested guards below");
  if (!AHEAD) {
    if (!KEEP) vw_load(gb.pvw, v, w);
    ground_point<WARM>(cg_load(rec, 0), gb, 0, ws, mu, v, w, res);        // (a body lane is called with np >= 1)
    if (gb.np > 1) {
      ground_point<WARM>(cg_load(rec, 1), gb, 1, ws, mu, v, w, res);
      if (gb.np > 2) {
        ground_point<WARM>(cg_load(rec, 2), gb, 2, ws, mu, v, w, res);
        if (gb.np > 3) ground_point<WARM>(cg_load(rec, 3), gb, 3, ws, mu, v, w, res);
      }
    }
  } else {
    const unsigned ra = (unsigned)(size_t)rec;   // the LDS byte address (the low word of the generic pointer)
    GRec r0, r1, r2, r3;
    if (!KEEP) {
      f4 a0; f2 a1;
      float none = 0.0f;
      cg_request_first((unsigned)(size_t)gb.pvw, ra, a0, a1, r0);
      cg_request<1>(ra, r1, none);
      cg_arrive_first(a0, a1, r0);
      v = V(a0.x, a0.z, a1.x); w = V(a0.y, a0.w, a1.y);
    } else {
      cg_request<0>(ra, r0, w.z);
      cg_request<1>(ra, r1, w.z);
      cg_arrive<5>(r0, w.z);
    }
    ground_point<WARM>(r0, gb, 0, ws, mu, v, w, res);
    cg_arrive<0>(r1, w.x);
    if (gb.np > 1) {
      cg_request<2>(ra, r2, w.z);
      ground_point<WARM>(r1, gb, 1, ws, mu, v, w, res);
      cg_arrive<0>(r2, w.x);
      if (gb.np > 2) {
        cg_request<3>(ra, r3, w.z);
        ground_point<WARM>(r2, gb, 2, ws, mu, v, w, res);
        cg_arrive<0>(r3, w.x);
        if (gb.np > 3) ground_point<WARM>(r3, gb, 3, ws, mu, v, w, res);
      }
    }
  }
  if (!KEEP) vw_store(gb.pvw, v, w);
}

__device__ __forceinline__ Point make_pair_point(const Lds& L, int sl, int i) {
  const DevParams& P = *L.P;
  Point p;
  p.valid = false; p.a = 0; p.b = 0; p.colour = 0; p.idx = i;
  p.in = 0.0f; p.i1 = 0.0f; p.i2 = 0.0f; p.target = 0.0f; p.ima = 0.0f; p.imb = 0.0f; p.mu = 0.0f;
  if (sl >= P.NS) return p;
  const int pid = L.POS()[sl];
  if (pid < 0) return p;
  const float* mp = L.MAN(sl);
  if (i >= __float_as_int(mp[0])) return p;
  p.valid = true;
  L.pair(pid, p.a, p.b);
  p.colour = L.COL()[sl];
  p.ima = L.BC(p.a)[0]; p.imb = L.BC(p.b)[0];
  p.mu = P.c.friction_rock * P.c.friction_rock;
  const float* q = mp + 4 + SRL_MP_WORDS * i;
  const m3 Ra = ldm(L.R(p.a)), Rb = ldm(L.R(p.b));
  const m3 Ia = ldm(L.IW(p.a)), Ib = ldm(L.IW(p.b));
  const v3 ra = mmul(Ra, ld3(q));
  const v3 rb = mmul(Rb, ld3(q + 3));
  v3 n = ld3(q + 6), t1, t2;
  plane_space(n, t1, t2);
  p.n = pack_row(make_row<true>(n, ra, rb, p.ima, Ia, p.imb, Ib), p.ima, p.imb);
  p.t1 = pack_row(make_row<true>(t1, ra, rb, p.ima, Ia, p.imb, Ib), p.ima, p.imb);
  p.t2 = pack_row(make_row<true>(t2, ra, rb, p.ima, Ia, p.imb, Ib), p.ima, p.imb);
  p.t1.rk = -p.t1.rk; p.t2.rk = -p.t2.rk;   // (prow_solve<FRICTION>)
  p.target = contact_target(P, q[9]);
  p.in = q[10]; p.i1 = q[11]; p.i2 = q[12];
  return p;
}

// one turn of a point: read the velocities of its bodies, three rows, write them back (the variants without PAIR_SPLIT: one lane
// in four of a slot's quad works in a turn and runs both bodies' halves of a row one after the other — 67 vector instructions,
// four LDS reads and four writes; they are throughput-bound and have no registers for a second set of rows)
template <bool WARM>
__device__ __forceinline__ void point_turn(const Lds& L, Point& p, float& res) {
  const float ws = L.P->c.warmstart;
  Vel2 u;
  float* const pa = L.VW(p.a);
  float* const pb = L.VW(p.b);
  vw_load(pa, u.a);
  vw_load(pb, u.b);
  if (WARM) {
    p.in = p.in * ws; p.i1 = p.i1 * ws; p.i2 = p.i2 * ws;
    prow_apply(p.n, u, p.in);
    prow_apply(p.t1, u, p.i1);
    prow_apply(p.t2, u, p.i2);
  } else {
    prow_solve<false>(p.n, u, p.target, p.in, 0.0f, 1e30f, res);
    const float lim = p.mu * p.in;
    prow_solve<true>(p.t1, u, 0.0f, p.i1, -lim, lim, res);
    prow_solve<true>(p.t2, u, 0.0f, p.i2, -lim, lim, res);
  }
  vw_store(pa, u.a);
  vw_store(pb, u.b);
}

// ---- the pair turn on TWO lanes, one per body (Variant::PAIR_SPLIT).  In point_turn one lane in four of a slot's quad works and
// runs the rows of body A and of body B one after the other: the two halves of a row are the same instruction sequence on
// different constants and meet in one sum.  Here the even lane of a lane pair holds body A's half of a row — k[c] = (d.c, ca.c),
// u[c] = (d.c ima, aa.c) — and the odd lane body B's with kb NEGATED — k[c] = (-d.c, -cb.c), u[c] = (d.c (-imb), -ab.c).
// Negation passes exactly through a product and an FMA chain, so the odd lane's s.x + s.y is exactly -(sb.x + sb.y) of
// prow_solve, and own + partner (one v_add_f32_dpp quad_perm:[1,0,3,2]; IEEE add commutes) is prow_solve's
// ra - (sb.x + sb.y) on both lanes.  dl, the med3, the accumulated impulse, lim and res are computed on both lanes, bit-equal;
// each lane applies its own body's three packed FMAs.  The effective mass (ima + ...) + (imb + ...) is formed from the two
// lanes' parts with the same add: make_row<true>'s tree.  Lanes (0, 1) of the quad take points 0 and 1 of the manifold, lanes
// (2, 3) points 2 and 3 — two register sets per lane, the turns unrolled — so a body's velocities stay in the lane's registers
// from a pair's first turn to its second: one LDS hand-off in two is gone, and no register moves.  Both lanes of a pair are in
// EXEC for every turn: membership comes from the slot's point count and colour, which the quad shares.
// A turn was 45 vector instructions with one LDS read and write per pair of turns (point_turn: 67, four reads and four writes
// per turn): +10.6 % at the headline shape for the split alone, +14.5 % with the velocities kept (profiles/pair_split_experiment.md).
// It is 43 now: a friction row's impulse is the plain product vrel (-rk) (hrow_solve<FRICTION>), and the product 0 rk that was
// made in front of each friction row as the FMA's addend is gone (profiles/ground_zero_terms_ab.txt).
struct HRow { f2 k[3], u[3]; float rk, kk; };   // one body's half of a row; kk = effective mass denominator, rk = 1 / kk (friction rows: -1 / kk)
struct HSet { HRow n, t1, t2; float trk, in, i1, i2; };   // trk = target rk of the normal row (a friction row's target is 0)
struct PSplit {
  HSet s0, s1;     // the lane pair's first and second point: points 2 h and 2 h + 1 of the manifold, h = (lane >> 1) & 1
  float* pvw;      // the lane's own body's velocities in LDS (Lds::VW)
  int np;          // contact points of the lane's slot (0: none)
  int colour;
  float mu;
};

__device__ __forceinline__ float quad_partner(float x) {   // the value of lane ^ 1
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true));
}

// side 0: body A's half, side 1: body B's.  Called by both lanes of a pair together (the effective mass needs the partner's part).
__device__ __forceinline__ HRow make_hrow(v3 d, v3 r, float im, const m3& I, bool side) {
  HRow h;
  const v3 c = cross(r, d);
  const v3 a = mmul(I, c);
  const float part = im + dot(cross(a, r), d);
  const float k = part + quad_partner(part);
  const v3 dm = d * (side ? -im : im);
  h.k[0] = side ? F2(-d.x, -c.x) : F2(d.x, c.x); h.k[1] = side ? F2(-d.y, -c.y) : F2(d.y, c.y); h.k[2] = side ? F2(-d.z, -c.z) : F2(d.z, c.z);
  h.u[0] = F2(dm.x, side ? -a.x : a.x); h.u[1] = F2(dm.y, side ? -a.y : a.y); h.u[2] = F2(dm.z, side ? -a.z : a.z);
  h.rk = 1.0f / k; h.kk = k;
  return h;
}

__device__ __forceinline__ HSet make_hset(const Lds& L, const float* mp, int i, int np, int body, bool side) {
  const DevParams& P = *L.P;
  HSet s;
  s.trk = 0.0f; s.in = 0.0f; s.i1 = 0.0f; s.i2 = 0.0f;
  if (i >= np) {   // (uniform over the lane pair)
    HRow z;
    z.k[0] = z.k[1] = z.k[2] = z.u[0] = z.u[1] = z.u[2] = F2(0.0f, 0.0f); z.rk = 0.0f; z.kk = 0.0f;
    s.n = z; s.t1 = z; s.t2 = z;
    return s;
  }
  const float im = L.BC(body)[0];
  const float* q = mp + 4 + SRL_MP_WORDS * i;
  const v3 r = mmul(ldm(L.R(body)), ld3(q + (side ? 3 : 0)));
  const m3 I = ldm(L.IW(body));
  v3 n = ld3(q + 6), t1, t2;
  plane_space(n, t1, t2);
  s.n = make_hrow(n, r, im, I, side);
  s.t1 = make_hrow(t1, r, im, I, side);
  s.t2 = make_hrow(t2, r, im, I, side);
  s.t1.rk = -s.t1.rk; s.t2.rk = -s.t2.rk;   // (hrow_solve<FRICTION>)
  s.trk = contact_target(P, q[9]) * s.n.rk;
  s.in = q[10]; s.i1 = q[11]; s.i2 = q[12];
  return s;
}

__device__ __forceinline__ int slot_points(const Lds& L, int sl) {   // contact points of slot sl (0: free, or past the last slot)
  if (sl >= L.P->NS || L.POS()[sl] < 0) return 0;
  return __float_as_int(L.MAN(sl)[0]);
}

__device__ __forceinline__ PSplit make_pair_split(const Lds& L, int tid) {
  const DevParams& P = *L.P;
  const int sl = tid >> 2, h = (tid >> 1) & 1;
  const bool side = tid & 1;
  PSplit p;
  p.np = 0; p.colour = 0; p.pvw = L.VW(0);
  p.mu = P.c.friction_rock * P.c.friction_rock;
  int body = 0;
  const float* mp = L.MAN(0);
  if (sl < P.NS) {
    const int pid = L.POS()[sl];
    if (pid >= 0) {
      int a, b; L.pair(pid, a, b);
      body = side ? b : a;
      mp = L.MAN(sl);
      p.np = __float_as_int(mp[0]);
      p.colour = L.COL()[sl];
      p.pvw = L.VW(body);
    }
  }
  p.s0 = make_hset(L, mp, 2 * h, p.np, body, side);
  p.s1 = make_hset(L, mp, 2 * h + 1, p.np, body, side);
  return p;
}

__device__ __forceinline__ void hrow_apply(const HRow& r, f2 (&u)[3], f2 d2) {   // d2: the impulse in both halves
#pragma unroll
  for (int c = 0; c < 3; ++c) u[c] = fma2(r.u[c], d2, u[c]);
}
template <bool FRICTION>   // FRICTION: target 0, r.rk = -1 / kk, dl = vrel (-rk) (as prow_solve)
__device__ __forceinline__ void hrow_solve(const HRow& r, f2 (&u)[3], float trk, float& acc, float lo, float hi, float& res) {
  const f2 s = fma2(r.k[0], u[0], fma2(r.k[1], u[1], r.k[2] * u[2]));   // A: (dot(d, va), dot(ca, wa)); B: minus its own
  float own = s.x + s.y;
  asm("" : "+v"(own));   // (kept from the vectoriser, as in prow_solve)
  const float vrel = own + quad_partner(own);
  float dl = FRICTION ? vrel * r.rk : fmaf(-vrel, r.rk, trk);
  const float na = __builtin_amdgcn_fmed3f(acc + dl, lo, hi);
  dl = na - acc;
  acc = na;
  res = fmaxf(res, fabsf(dl * r.kk));
  hrow_apply(r, u, F2(dl, dl));
}

// one turn of a lane pair on one of its points: three rows on the two bodies' velocities, each in its lane's registers
template <bool WARM>
__device__ __forceinline__ void hset_turn(HSet& s, f2 (&u)[3], float mu, float ws, float& res) {
  if (WARM) {
    s.in = s.in * ws; s.i1 = s.i1 * ws; s.i2 = s.i2 * ws;
    const f2 dn = F2(s.in, s.in), d1 = F2(s.i1, s.i1), d2 = F2(s.i2, s.i2);   // (made first: the order the kernel was tuned in)
    hrow_apply(s.n, u, dn);
    hrow_apply(s.t1, u, d1);
    hrow_apply(s.t2, u, d2);
  } else {
    hrow_solve<false>(s.n, u, s.trk, s.in, 0.0f, 1e30f, res);
    const float lim = mu * s.in;
    hrow_solve<true>(s.t1, u, 0.0f, s.i1, -lim, lim, res);
    hrow_solve<true>(s.t2, u, 0.0f, s.i2, -lim, lim, res);
  }
}

// One colour's phase.  m1 / m2: the colour's lanes whose pair holds a first / a second point (a lane's pair: np > 2 h and
// np > 2 h + 1), as wave-uniform masks.  Lanes (0, 1) of the quads, then lanes (2, 3); the phase ends at its first empty turn.
// A pair's second turn runs inside its first's guard, on the velocities the first left in registers: one read and one write
// of LDS per pair and phase.  (With a read and a write around every turn — the split alone — the headline shape gained
// 10.6 %, with the velocities kept 14.5 %: profiles/pair_split_ab.txt.)
template <bool WARM>
__device__ __forceinline__ void pair_phase(PSplit& p, float ws, unsigned long long m1, unsigned long long m2, float& res) {
  constexpr unsigned long long LO = 0x3333333333333333ull;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const unsigned long long t1 = m1 & (LO << (2 * h)), t2 = m2 & (LO << (2 * h));
    if (t1 == 0) return;
    if (__builtin_amdgcn_inverse_ballot_w64(t1)) {
      f2 u[3];
      vw_load(p.pvw, u);
      hset_turn<WARM>(p.s0, u, p.mu, ws, res);
      if (t2 != 0) {
        if (__builtin_amdgcn_inverse_ballot_w64(t2)) hset_turn<WARM>(p.s1, u, p.mu, ws, res);
      }
      vw_store(p.pvw, u);
    }
    __builtin_amdgcn_wave_barrier();
    if (t2 == 0) return;
  }
}

// A wave runs only the turns it has points for (a turn no lane takes still costs a lone wave its control flow: 8 + 4 ncol empty
// turns per sweep were a third of the sub-step's instructions in round 1; rounds 2 - 5 counted the turns per phase / per colour,
// now a phase ends at its first empty mask).
// A sweep ends with a block barrier; before it every wave that still holds a row whose squared residual exceeds the
// threshold writes the sweep's number `gsweep` (counted over the whole launch, so a stale word never matches) into the
// LDS word of the sweep's parity; after the barrier every thread reads that word: `true` = some row has not converged
// (Bullet's m_leastSquaresResidual > m_leastSquaresResidualThreshold; the maximum over rows is order-independent, so
// the parallel sweep decides exactly as the sequential definition).  The word of the other parity is the one the
// next sweep writes, so a fast wave cannot disturb a slow wave's read.
// PAIR_SPLIT (srl_k_step): a colour's phase is pair_phase — lanes (0, 1) of the colour's quads on their two points, then lanes
// (2, 3) — under the same kind of scalar masks, made from the slot's point count and colour (a lane's own point does not exist:
// both lanes of a pair must be in EXEC for a turn); solo and barrier sweeps share it.  8.22 against 9.42 ms per launch.
// SOLO: every contact point of the env sits in wave 0 (the common case with few rocks: the ground points are the first
// lanes, and manifold slots are handed out lowest first), so the sweep is wave 0's alone: the phases follow each other in
// program order — the LDS serves one wave's accesses in order — without a single block barrier, and the residual is a
// ballot.  The other waves skip the sweeps and wait at the barrier that ends the solve.
template <bool WARM, int T, int PP, bool SOLO>
__device__ __forceinline__ bool solver_sweep(const Lds& L, GPoint& gp, GBody& gb, Point (&pp)[PP], PSplit& sp, int ncol, int gslot,
                                             const int (&pslot)[PP], int gsweep, const unsigned long long (&cm)[2],
                                             const unsigned long long (&cm2)[2], float gmu) {
  // gslot / pslot: the turn a lane's point takes (ground: its index; colour phases: 4 * colour + index; -1: none)
  // PAIR_SPLIT: sp instead of pp / pslot; cm / cm2: the first two colours' lanes whose pair holds a first / a second point
  // gmu: the ground points' friction coefficient (substep makes it once: read here, its scalar load would be waited for in
  // front of the first ground point, and the record requested ahead with it)
  typedef Variant<T, PP> VA;
  static_assert(!SOLO || VA::SOLO, "a solo sweep in a variant that has none");
  float res = 0.0f;
  // A turn's guard is a SCALAR mask: a point's index in its manifold is its lane & 3 (four consecutive lanes per body / per slot), so
  // turn i of a phase is (the phase's lanes) & 0x1111... << i — `s_and_b64` + `s_and_saveexec_b64` on a uniform value
  // (inverse ballot).  As a vector compare per turn inside a rolled loop the guard and the loop's backward branch cost a lone wave
  // ≈ 75 cycles a turn (microbenchmark: compare -> VCC -> exec 32 cycles, a taken branch ≈ 32): the turns are unrolled, a
  // phase ends at its first empty turn (the points of a manifold are a prefix).
  constexpr unsigned long long T0 = 0x1111111111111111ull;
  if (!VA::GROUND_BODY) {     // the points of a body as turns of point lanes (round 1 - 4; kept for the variant that loses with body lanes)
    const unsigned long long gm = __ballot(gslot >= 0);
#pragma unroll
    for (int i = 0; i < SRL_GMAXP; ++i) {
      const unsigned long long t = gm & (T0 << i);
      if (t == 0) break;
      if (__builtin_amdgcn_inverse_ballot_w64(t)) ground_turn<WARM>(L, gp, gmu, res);
      __builtin_amdgcn_wave_barrier();
    }
  } else {
    v3 v, w;
    if (gb.np > 0) ground_body<WARM, !WARM && VA::GROUND_AHEAD, false>(gb, L.P->c.warmstart, gmu, v, w, res);
    __builtin_amdgcn_wave_barrier();
  }
  int c0 = 0;
  if (SOLO) {   // the first two colours from masks made once per sub-step, straight-line (no ballot, no loop branch per colour)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (c >= ncol) break;
      if constexpr (VA::PAIR_SPLIT) {
        pair_phase<WARM>(sp, L.P->c.warmstart, cm[c], cm2[c], res);
      } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned long long t = cm[c] & (T0 << i);
        if (t == 0) break;
        if (__builtin_amdgcn_inverse_ballot_w64(t)) point_turn<WARM>(L, pp[0], res);
        __builtin_amdgcn_wave_barrier();
      }
      }
    }
    c0 = 2;
  }
#pragma unroll 1
  for (int c = c0; c < ncol; ++c) {
    if (!SOLO) __syncthreads();
    if constexpr (VA::PAIR_SPLIT) {
      const int h2 = (threadIdx.x >> 1) & 1;
      const bool mine = sp.colour == c;
      pair_phase<WARM>(sp, L.P->c.warmstart, __ballot(mine && sp.np > 2 * h2), __ballot(mine && sp.np > 2 * h2 + 1), res);
    } else {
    unsigned long long mc[PP];
#pragma unroll
    for (int r = 0; r < PP; ++r) mc[r] = __ballot((pslot[r] >> 2) == c);   // (pslot = -1: no point)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned long long any = 0;
#pragma unroll
      for (int r = 0; r < PP; ++r) any |= mc[r] & (T0 << i);
      if (any == 0) break;
#pragma unroll
      for (int r = 0; r < PP; ++r)
        if (__builtin_amdgcn_inverse_ballot_w64(mc[r] & (T0 << i))) point_turn<WARM>(L, pp[r], res);
      __builtin_amdgcn_wave_barrier();
    }
    }
  }
  if (SOLO) return WARM ? true : __ballot(res * res > L.P->c.residual_threshold) != 0ull;
  int* word = L.MISC() + M_RES0 + (gsweep & 1);
  if (!WARM) {
    if (__ballot(res * res > L.P->c.residual_threshold) != 0ull && (threadIdx.x & 63) == 0) *word = gsweep;
  }
  __syncthreads();
  return WARM ? true : *word == gsweep;
}
