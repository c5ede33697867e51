// float_plan.h -- Lagrangian floats advected through the resident state (hnumo_floats_*).
//
// Plain C++17, no HIP call: engine.hip and kernels_float.hip include it for the engine,
// tests/float_plan_main.cpp for a CPU program that runs under the host sanitizers
// (tests/test_float_plan.py).  It reuses sample_plan.h: the bilinear map, its Newton inverse, the
// Lagrange weights and the initial location are the sample sets'.
//
// A float set is M floats.  A float carries a physical position (x, y), a layer k (1-based, fixed),
// a stored velocity w = (wx, wy), a cached location (elem, xi, eta) and a status (0 ACTIVE, 1 LEFT --
// also "not on this rank at creation" --, 2 LOST).  All arithmetic is IEEE double, no FMA
// (-ffp-contract=off), IEEE division.
//
// Velocity of layer k at (e, xi, eta) (float_vel): nodal U(I) = q(2,I,k)/q(1,I,k), V(I) = q(3,I,k)/
//   q(1,I,k), I = e*P + j*ngl + i; weights Lx, Ly by sample_weights' rule; value = sum_j Ly[j] *
//   (sum_i Lx[i] * U), both sums left to right from their first product: rows 5(k-1)+2, 5(k-1)+3 of
//   a hnumo_sample_create_ref set at (elem, xi, eta).
// Location of a target p starting from element e (float_locate):
//   1. invert e's bilinear map at p with sample_invert's loop (float_invert: the same statements);
//      no finite solution: LOST;
//   2. max(|xi|, |eta|) <= 1 + tol_e: clamp both to [-1,1] and accept;
//   3. otherwise the side with the larger excess (|xi| - 1 against |eta| - 1, a tie goes to xi; the
//      sign selects the face): an owned neighbour -> e = neighbour, go to 1; a physical boundary ->
//      that coordinate = +-1 exactly, p = e's bilinear map at the new (xi, eta) (the float slides
//      along the wall), go to 1 in the same element; a processor face or a ghost neighbour -> LEFT;
//   4. each pass through 3 is a hop; a fifth hop: LOST.
// Advance by dt (float_advance): Heun with the field of the new time level, w from the previous:
//   if fresh: w = vel(elem, xi, eta), fresh = 0
//   p* = (x + dt*wx, y + dt*wy);  (e*, xi*, eta*, p*) = locate(p*, elem);  u* = vel(e*, xi*, eta*)
//   p1 = (x + (0.5*dt)*(wx + u*x), y + (0.5*dt)*(wy + u*y));  (e1, ..) = locate(p1, e*)
//   w = vel(e1, xi1, eta1);  (x, y) = p1;  (elem, xi, eta) = (e1, xi1, eta1)
//   A location that ends LEFT or LOST stops the advance: (x, y) = that location's target, elem = 0,
//   w = 0.  A non-finite velocity gives LOST the same way, (x, y) = the target located last (the
//   float's own (x, y) for the fresh evaluation).  Inactive floats are never touched again.
// Every loop is bounded: 32 Newton iterations, 4 hops.
//
// Migration (processor-face ranks; include/hnumo_engine.h has the normative text).  In a migrating set
// a location that reaches step 3 at a processor face returns FL_FLIGHT and fills a FloatFlight: the
// float's (x, y, w) at the start of this advance, dt, the stage (0 locating p*, 1 locating p1), the
// current target, the passes through 3 so far and the destination (k, pos) = (neighbour index, position
// of the face in that neighbour's list).  The sender's slot becomes LEFT as before.  float_resume runs
// the tail of the advance on the receiver from the element behind the face; MIG is a template flag, so
// float_advance<NGL> is the text it was.
//
// The host part: the per-element tables (corners [E][4][2], tol_e [E], side neighbours [E][4] with
// sides xi=-1, xi=+1, eta=-1, eta=+1: neighbour element, -1 wall, -2 off-rank), derived from face,
// imapl, imapr by the set of local nodes on each side; validation (every failure: code 4 and a
// message); the initial location through sample_locate; the stable sort by initial element; for migrating
// sets the side table xface, the arrival table and the inverse permutation (float_xface,
// float_inverse_perm), tol_e under a coord_scale (float_tolerances) and the host statements of the
// two kernels (float_advance_mig_ngl, float_arrive_ngl).
#pragma once
#include <type_traits>

#include "sample_plan.h"

#if defined(__HIPCC__)
#define HNUMO_HD __host__ __device__
#else
#define HNUMO_HD
#endif

namespace hnumo {

constexpr int FL_MAXSETS = 8;
constexpr int FL_BLOCK = 256;                       // lanes of the kernels' workgroup
constexpr int FL_ACTIVE = 0, FL_LEFT = 1, FL_LOST = 2;
constexpr int FL_WALL = -1, FL_OFF_RANK = -2;       // side neighbours that are no element
constexpr int FL_MAXHOPS = 4, FL_NEWTON = 32;
constexpr int FL_NREC = 5;                          // a record: x, y, u, v, elem
constexpr int FL_FLIGHT = 3;                        // float_locate<true>'s answer at a processor face (never a float's status)
constexpr int FL_MAXROUNDS = 8;                     // rounds of arrivals that settle one advance (2 locations x 4 hops)
constexpr int FL_FD = 7, FL_FI = 6;                 // double and int32 planes of an outbox

// what the three functions read: the tables of the owned elements and the state
struct FloatField {
  const double *corners;      // [E][4][2]
  const double *tol;          // [E]
  const int32_t *nbr;         // [E][4]
  const double *q;            // q_df(3, npoin, L)
  size_t npoin;
  double xgl[8];
};

// one float, in registers
struct FloatRec {
  double x, y, wx, wy, xi, eta;
  int32_t elem, layer, status, fresh;
};

// a float in flight between two ranks (planes of an outbox: x, y, wx, wy, dt, px, py | gid, layer, stage,
// hops, k, pos)
struct FloatFlight {
  double x, y, wx, wy, dt, px, py;
  int32_t gid, layer, stage, hops, k, pos;
};

HNUMO_HD inline bool float_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }   // (false for a NaN)

// sample_bilinear on corners c[8] = [4][2]
HNUMO_HD inline void float_bilinear(const double *c, double xi, double eta, double (&x)[2], double (*J)[2]) {
  const double w[4] = {0.25 * (1 - xi) * (1 - eta), 0.25 * (1 + xi) * (1 - eta), 0.25 * (1 + xi) * (1 + eta),
                       0.25 * (1 - xi) * (1 + eta)};
  for (int d = 0; d < 2; d++) x[d] = w[0] * c[d] + w[1] * c[2 + d] + w[2] * c[4 + d] + w[3] * c[6 + d];
  if (J)
    for (int d = 0; d < 2; d++) {
      J[d][0] = 0.25 * (-(1 - eta) * c[d] + (1 - eta) * c[2 + d] + (1 + eta) * c[4 + d] - (1 + eta) * c[6 + d]);
      J[d][1] = 0.25 * (-(1 - xi) * c[d] - (1 + xi) * c[2 + d] + (1 + xi) * c[4 + d] + (1 - xi) * c[6 + d]);
    }
}

// sample_invert's loop
HNUMO_HD inline bool float_invert(const double *c, double px, double py, double &xi, double &eta) {
  xi = eta = 0.0;
  for (int it = 0; it < FL_NEWTON; it++) {
    double x[2], J[2][2];
    float_bilinear(c, xi, eta, x, J);
    const double rx = px - x[0], ry = py - x[1];
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double dxi = (J[1][1] * rx - J[0][1] * ry) / det, deta = (J[0][0] * ry - J[1][0] * rx) / det;
    if (!float_finite(dxi) || !float_finite(deta)) return false;
    xi += dxi;
    eta += deta;
    if (__builtin_fabs(xi) > 1e3 || __builtin_fabs(eta) > 1e3) return false;
    if (__builtin_fabs(dxi) <= 1e-16 && __builtin_fabs(deta) <= 1e-16) break;
  }
  return true;
}

// (u, v) of layer k (0-based) at (e, xi, eta), e 0-based
template <int NGL>
HNUMO_HD inline void float_vel(const FloatField &f, int k, int e, double xi, double eta, double &u, double &v) {
  double lx[NGL], ly[NGL];
#pragma unroll
  for (int i = 0; i < NGL; i++) {
    double wx = 1.0, wy = 1.0;
#pragma unroll
    for (int m = 0; m < NGL; m++)
      if (m != i) {
        wx = wx * ((xi - f.xgl[m]) / (f.xgl[i] - f.xgl[m]));
        wy = wy * ((eta - f.xgl[m]) / (f.xgl[i] - f.xgl[m]));
      }
    lx[i] = wx;
    ly[i] = wy;
  }
  const double *p = f.q + 3 * ((size_t)e * (NGL * NGL) + f.npoin * (size_t)k);
  u = v = 0.0;
#pragma unroll
  for (int j = 0; j < NGL; j++) {
    const double *r = p + 3 * j * NGL;
    double ru = lx[0] * (r[1] / r[0]), rv = lx[0] * (r[2] / r[0]);
#pragma unroll
    for (int i = 1; i < NGL; i++) {
      ru = ru + lx[i] * (r[3 * i + 1] / r[3 * i]);
      rv = rv + lx[i] * (r[3 * i + 2] / r[3 * i]);
    }
    u = j == 0 ? ly[0] * ru : u + ly[j] * ru;
    v = j == 0 ? ly[0] * rv : v + ly[j] * rv;
  }
}

// locates (px, py) starting from element e (0-based); on return the element, its clamped (xi, eta)
// and the target, which a wall may have moved.  Returns the status.  `hop`: the passes through 3 behind
// this location (an arrival's).  MIG: a processor face listed in xface [E][4][2] gives FL_FLIGHT with
// the target, the passes so far and (k, pos) in *fl.
template <bool MIG = false>
HNUMO_HD inline int float_locate(const FloatField &f, double &px, double &py, int &e, double &xi, double &eta, int hop = 0,
                                 const int32_t *xface = nullptr, FloatFlight *fl = nullptr) {
  for (;; hop++) {
    const double *c = f.corners + 8 * (size_t)e;
    if (!float_invert(c, px, py, xi, eta)) return FL_LOST;
    const double ax = __builtin_fabs(xi), ay = __builtin_fabs(eta);
    if ((ax < ay ? ay : ax) <= 1.0 + f.tol[e]) {
      xi = xi > 1.0 ? 1.0 : xi < -1.0 ? -1.0 : xi;
      eta = eta > 1.0 ? 1.0 : eta < -1.0 ? -1.0 : eta;
      return FL_ACTIVE;
    }
    if (hop == FL_MAXHOPS) return FL_LOST;
    const bool in_eta = ay - 1.0 > ax - 1.0;
    const bool plus = (in_eta ? eta : xi) > 0.0;
    const int nb = f.nbr[4 * (size_t)e + (in_eta ? 2 : 0) + (plus ? 1 : 0)];
    if (nb >= 0) {
      e = nb;
    } else if (nb == FL_WALL) {
      (in_eta ? eta : xi) = plus ? 1.0 : -1.0;
      double x[2];
      float_bilinear(c, xi, eta, x, nullptr);
      px = x[0];
      py = x[1];
    } else {
      if constexpr (MIG) {
        const int32_t *d = xface + 2 * (4 * (size_t)e + (in_eta ? 2 : 0) + (plus ? 1 : 0));
        if (d[0] >= 0) {
          fl->px = px;
          fl->py = py;
          fl->hops = hop + 1;
          fl->k = d[0];
          fl->pos = d[1];
          return FL_FLIGHT;
        }
      }
      return FL_LEFT;
    }
  }
}

HNUMO_HD inline void float_stop(FloatRec &r, int status, double px, double py) {
  r.status = status;
  r.x = px;
  r.y = py;
  r.elem = 0;
  r.wx = r.wy = 0.0;
}

// how an evaluation is carried out: by the lane (or host thread) itself; the kernel has a second way
struct FloatVelPlain {
  template <int NGL>
  HNUMO_HD void eval(const FloatField &f, int k, int e, double xi, double eta, double &u, double &v) const {
    float_vel<NGL>(f, k, e, xi, eta, u, v);
  }
};

// a location of stage `stage` ended with st != ACTIVE: the slot stops; true: the float is in flight (*fl complete
// but for gid)
template <bool MIG>
HNUMO_HD inline bool float_leave(FloatRec &r, int st, double px, double py, double dt, int stage, FloatFlight *fl) {
  if constexpr (MIG)
    if (st == FL_FLIGHT) {
      fl->x = r.x;
      fl->y = r.y;
      fl->wx = r.wx;
      fl->wy = r.wy;
      fl->dt = dt;
      fl->layer = r.layer;
      fl->stage = stage;
      float_stop(r, FL_LEFT, px, py);
      return true;
    }
  float_stop(r, st, px, py);
  return false;
}

// float_advance's statements from a stage on, for a float that arrives (the same text, statement for statement:
// float_advance itself stays the straight-line text its kernel has always been compiled from).  Stage 0: locate p* = (px, py) from e with `hop` passes
// behind it, u* = vel, p1, and go on as stage 1 from there with no pass behind; stage 1: locate p1 = (px, py),
// w = vel, the float moves.  True: in flight (MIG only).
template <int NGL, class Vel>
HNUMO_HD inline bool float_heun(const FloatField &f, double dt, FloatRec &r, const Vel &vel, int stage, double px, double py, int e,
                                int hop, const int32_t *xface, FloatFlight *fl) {
  const int k = r.layer - 1;
  double xi, eta;
  if (stage == 0) {
    const int st = float_locate<true>(f, px, py, e, xi, eta, hop, xface, fl);
    if (st != FL_ACTIVE) return float_leave<true>(r, st, px, py, dt, 0, fl);
    double us, vs;
    vel.template eval<NGL>(f, k, e, xi, eta, us, vs);
    if (!float_finite(us) || !float_finite(vs)) return float_stop(r, FL_LOST, px, py), false;
    px = r.x + (0.5 * dt) * (r.wx + us);
    py = r.y + (0.5 * dt) * (r.wy + vs);
    hop = 0;
  }
  const int st = float_locate<true>(f, px, py, e, xi, eta, hop, xface, fl);
  if (st != FL_ACTIVE) return float_leave<true>(r, st, px, py, dt, 1, fl);
  double us, vs;
  vel.template eval<NGL>(f, k, e, xi, eta, us, vs);
  if (!float_finite(us) || !float_finite(vs)) return float_stop(r, FL_LOST, px, py), false;
  r.x = px;
  r.y = py;
  r.wx = us;
  r.wy = vs;
  r.elem = e + 1;
  r.xi = xi;
  r.eta = eta;
  return false;
}

template <int NGL, bool MIG = false, class Vel>
HNUMO_HD inline bool float_advance(const FloatField &f, double dt, FloatRec &r, const Vel &vel, const int32_t *xface = nullptr,
                                   FloatFlight *fl = nullptr) {
  if (r.status != FL_ACTIVE) return false;
  const int k = r.layer - 1;
  int e = r.elem - 1;
  if (r.fresh) {
    vel.template eval<NGL>(f, k, e, r.xi, r.eta, r.wx, r.wy);
    r.fresh = 0;
    if (!float_finite(r.wx) || !float_finite(r.wy)) return float_stop(r, FL_LOST, r.x, r.y), false;
  }
  double px = r.x + dt * r.wx, py = r.y + dt * r.wy, xi, eta;
  int st = float_locate<MIG>(f, px, py, e, xi, eta, 0, xface, fl);
  if (st != FL_ACTIVE) return float_leave<MIG>(r, st, px, py, dt, 0, fl);
  double us, vs;
  vel.template eval<NGL>(f, k, e, xi, eta, us, vs);
  if (!float_finite(us) || !float_finite(vs)) return float_stop(r, FL_LOST, px, py), false;
  px = r.x + (0.5 * dt) * (r.wx + us);
  py = r.y + (0.5 * dt) * (r.wy + vs);
  st = float_locate<MIG>(f, px, py, e, xi, eta, 0, xface, fl);
  if (st != FL_ACTIVE) return float_leave<MIG>(r, st, px, py, dt, 1, fl);
  vel.template eval<NGL>(f, k, e, xi, eta, us, vs);
  if (!float_finite(us) || !float_finite(vs)) return float_stop(r, FL_LOST, px, py), false;
  r.x = px;
  r.y = py;
  r.wx = us;
  r.wy = vs;
  r.elem = e + 1;
  r.xi = xi;
  r.eta = eta;
  return false;
}

// The tail of an advance from a flight record, on the rank across the face: e (0-based) is the element behind
// it.  r comes in as the receiver's slot (its xi, eta, elem stay if the float does not settle here) and leaves
// as the float; true: in flight again, *fl complete but for gid.
template <int NGL, class Vel>
HNUMO_HD inline bool float_resume(const FloatField &f, const int32_t *xface, const FloatFlight &in, int e, FloatRec &r, const Vel &vel,
                                  FloatFlight *fl) {
  r.x = in.x;
  r.y = in.y;
  r.wx = in.wx;
  r.wy = in.wy;
  r.layer = in.layer;
  r.status = FL_ACTIVE;
  r.fresh = 0;
  return float_heun<NGL>(f, in.dt, r, vel, in.stage, in.px, in.py, e, in.hops, xface, fl);
}

// ------------------------------------------------------------------ the host part
inline bool float_ngl_ok(int ngl) { return ngl == 3 || ngl == 4 || ngl == 5 || ngl == 6 || ngl == 8; }

// the side (0..3: xi=-1, xi=+1, eta=-1, eta=+1) all ngl nodes of face f lie on in imap(3,ngl,nface); -1 none, 4 several
inline int float_face_side(const int32_t *imap, int ngl, int f) {
  bool all[4] = {true, true, true, true};
  for (int n = 0; n < ngl; n++) {
    const int32_t i = imap[3 * ((size_t)n + (size_t)ngl * f)], j = imap[3 * ((size_t)n + (size_t)ngl * f) + 1];
    all[0] = all[0] && i == 1;
    all[1] = all[1] && i == ngl;
    all[2] = all[2] && j == 1;
    all[3] = all[3] && j == ngl;
  }
  int s = -1;
  for (int t = 0; t < 4; t++)
    if (all[t]) s = s < 0 ? t : 4;
  return s;
}

// Side neighbours [nelem_owned][4] from face(8,nface), imapl, imapr (3,ngl,nface): the side of an
// element that a face lies on is read from the local nodes the face lists for that element (all
// i = 1: xi = -1; all i = ngl: xi = +1; all j = 1: eta = -1; all j = ngl: eta = +1), whatever the
// mesher's local face numbering and whichever way the two elements meet.
inline int float_side_neighbours(const int32_t *face, const int32_t *imapl, const int32_t *imapr, int nface, int ngl, int nelem,
                                 int nelem_owned, std::vector<int32_t> &nbr, std::string &err) {
  const char *who = "hnumo_floats_create";
  if (!face || !imapl || !imapr) return err = std::string(who) + ": face, imapl or imapr is NULL", SP_ERR_INVALID;
  if (ngl < 2 || nelem_owned < 0 || nelem_owned > nelem)
    return err = std::string(who) + ": ngl must be >= 2 and nelem_owned in 0..nelem", SP_ERR_INVALID;
  const int32_t UNSET = -3;
  nbr.assign(4 * (size_t)nelem_owned, UNSET);
  for (int f = 0; f < nface; f++) {
    const int32_t el = face[8 * (size_t)f + 6], er = face[8 * (size_t)f + 7];
    if (el < 1 || el > nelem || er > nelem)
      return err = std::string(who) + ": face(7:8) of face " + std::to_string(f + 1) + " is out of range", SP_ERR_INVALID;
    for (int lr = 0; lr < 2; lr++) {
      const int32_t me = lr == 0 ? el : er, other = lr == 0 ? er : el;
      if (me < 1 || me > nelem_owned) continue;     // (a wall or processor face has no right element; ghosts hold no floats)
      const int s = float_face_side(lr == 0 ? imapl : imapr, ngl, f);
      if (s < 0 || s > 3)
        return err = std::string(who) + ": the nodes of face " + std::to_string(f + 1) + " are not one side of element " +
                     std::to_string(me),
               SP_ERR_INVALID;
      int32_t &slot = nbr[4 * (size_t)(me - 1) + s];
      if (slot != UNSET)
        return err = std::string(who) + ": two faces on one side of element " + std::to_string(me) +
                     " (non-conforming faces are not supported)",
               SP_ERR_INVALID;
      slot = lr == 1 ? (other <= nelem_owned ? other - 1 : FL_OFF_RANK)
                     : er < 0 ? FL_WALL : er == 0 ? FL_OFF_RANK : er <= nelem_owned ? er - 1 : FL_OFF_RANK;
    }
  }
  for (size_t t = 0; t < nbr.size(); t++)
    if (nbr[t] == UNSET)
      return err = std::string(who) + ": element " + std::to_string(t / 4 + 1) + " has a side without a face", SP_ERR_INVALID;
  return 0;
}

// the tables of the owned elements
struct FloatGeom {
  int ngl = 0, ne = 0;
  double maxc = 0.0;
  std::vector<double> corners, tol;   // [E][4][2], [E]
  std::vector<int32_t> nbr;           // [E][4]
  std::vector<double> coord, xgl;     // coord(2, ne*P) and xgl(ngl): what hnumo_floats_set locates in
};

// A set in the kernel's order s = 0..M-1: sorted stably by initial element; perm[s] = input position.
struct FloatPlan {
  int64_t M = 0;
  std::vector<int32_t> perm;
  std::vector<double> x, y, wx, wy, xi, eta;
  std::vector<int32_t> elem, layer, status, fresh;
  void get(size_t s, FloatRec &r) const {
    r = FloatRec{x[s], y[s], wx[s], wy[s], xi[s], eta[s], elem[s], layer[s], status[s], fresh[s]};
  }
  void put(size_t s, const FloatRec &r) {
    x[s] = r.x, y[s] = r.y, wx[s] = r.wx, wy[s] = r.wy, xi[s] = r.xi, eta[s] = r.eta;
    elem[s] = r.elem, layer[s] = r.layer, status[s] = r.status, fresh[s] = r.fresh;
  }
};

// tol_e of every element for max|coord| = maxc: (64 eps maxc) / (0.5 * shortest edge), float_geometry's own statement
inline void float_tolerances(const std::vector<double> &corners, double maxc, std::vector<double> &tol) {
  const double tol_x = 64.0 * std::numeric_limits<double>::epsilon() * maxc;
  tol.resize(corners.size() / 8);
  for (size_t e = 0; e < tol.size(); e++) {
    const double *c = corners.data() + 8 * e;
    double smin = INFINITY;
    for (int m = 0; m < 4; m++) {
      const double ex = c[2 * ((m + 1) & 3)] - c[2 * m], ey = c[2 * ((m + 1) & 3) + 1] - c[2 * m + 1];
      smin = std::min(smin, std::sqrt(ex * ex + ey * ey));
    }
    tol[e] = tol_x / (0.5 * smin);
  }
}

// corners, tol_e (sample_locate's) and the kept coord / xgl.  The bilinear-element contract and the
// rest of the geometry's validation are sample_locate's own, run by float_seed.
inline int float_geometry(const double *coord, int ldc, const double *xgl, int ngl, int nelem_owned,
                          const std::vector<int32_t> &nbr, FloatGeom &g, std::string &err) {
  const char *who = "hnumo_floats_create";
  if (!coord) return err = std::string(who) + ": coord is NULL", SP_ERR_INVALID;
  if (ldc != 2 && ldc != 3)
    return err = std::string(who) + ": ldc must be 2 or 3 (coord(ldc,npoin)), got " + std::to_string(ldc), SP_ERR_INVALID;
  if (!float_ngl_ok(ngl)) return err = std::string(who) + ": unsupported ngl " + std::to_string(ngl), SP_ERR_INVALID;
  if (int rc = sample_check_xgl(xgl, ngl, who, err)) return rc;
  if (nelem_owned < 0 || nbr.size() != 4 * (size_t)nelem_owned)
    return err = std::string(who) + ": the side neighbours do not cover the owned elements", SP_ERR_INVALID;
  const int ne = nelem_owned, P = ngl * ngl;
  g.ngl = ngl;
  g.ne = ne;
  g.nbr = nbr;
  g.xgl.assign(xgl, xgl + ngl);
  g.coord.resize(2 * (size_t)ne * P);
  double maxc = 0.0;
  for (size_t I = 0; I < (size_t)ne * P; I++)
    for (int d = 0; d < 2; d++) {
      const double c = coord[(size_t)ldc * I + d], v = std::fabs(c);
      if (!(v <= std::numeric_limits<double>::max()))
        return err = std::string(who) + ": coord is not finite at node " + std::to_string(I + 1), SP_ERR_INVALID;
      g.coord[2 * I + d] = c;
      maxc = std::max(maxc, v);
    }
  g.maxc = maxc;
  const double tol_x = 64.0 * std::numeric_limits<double>::epsilon() * maxc;
  g.corners.resize(8 * (size_t)ne);
  g.tol.resize(ne);
  for (int e = 0; e < ne; e++) {
    double c[4][2];
    sample_corners(g.coord.data(), 2, ngl, e, c);
    double smin = INFINITY;
    for (int m = 0; m < 4; m++) {
      const double ex = c[(m + 1) & 3][0] - c[m][0], ey = c[(m + 1) & 3][1] - c[m][1];
      smin = std::min(smin, std::sqrt(ex * ex + ey * ey));
      g.corners[8 * (size_t)e + 2 * m] = c[m][0];
      g.corners[8 * (size_t)e + 2 * m + 1] = c[m][1];
    }
    if (!(smin > 0.0))
      return err = std::string(who) + ": element " + std::to_string(e + 1) + " has an edge of length 0", SP_ERR_INVALID;
    g.tol[e] = tol_x / (0.5 * smin);
  }
  return 0;
}

// Seeds (or re-seeds) a set: xy(2,M), layer(M) in 1..nlayers; located through sample_locate; floats no
// owned element accepts are LEFT; w = 0, fresh = 1; sorted stably by element.
inline int float_seed(const FloatGeom &g, int nlayers, const double *xy, const int32_t *layer, int64_t M, FloatPlan &p,
                      std::string &err, const char *who = "hnumo_floats_create") {
  if (!xy) return err = std::string(who) + ": xy is NULL", SP_ERR_INVALID;
  if (!layer) return err = std::string(who) + ": layer is NULL", SP_ERR_INVALID;
  if (M < 1 || M > (int64_t)std::numeric_limits<int32_t>::max())
    return err = std::string(who) + ": M must be >= 1 (and < 2^31), got " + std::to_string(M), SP_ERR_INVALID;
  for (int64_t m = 0; m < M; m++)
    if (layer[m] < 1 || layer[m] > nlayers)
      return err = std::string(who) + ": layer(" + std::to_string(m + 1) + ") = " + std::to_string(layer[m]) + " is outside 1.." +
                   std::to_string(nlayers),
             SP_ERR_INVALID;
  SamplePlan sp;
  if (int rc = sample_locate(g.coord.data(), 2, g.xgl.data(), g.ngl, g.ne, xy, M, sp, err, who)) return rc;
  p.M = M;
  p.perm.resize(M);
  for (int64_t m = 0; m < M; m++) p.perm[m] = (int32_t)m;
  std::stable_sort(p.perm.begin(), p.perm.end(), [&](int32_t a, int32_t b) { return sp.elem[a] < sp.elem[b]; });
  for (std::vector<double> *v : {&p.x, &p.y, &p.wx, &p.wy, &p.xi, &p.eta}) v->assign(M, 0.0);
  for (std::vector<int32_t> *v : {&p.elem, &p.layer, &p.status, &p.fresh}) v->assign(M, 0);
  for (int64_t s = 0; s < M; s++) {
    const int64_t m = p.perm[s];
    p.x[s] = xy[2 * m];
    p.y[s] = xy[2 * m + 1];
    p.xi[s] = sp.xi_eta[2 * m];
    p.eta[s] = sp.xi_eta[2 * m + 1];
    p.elem[s] = sp.elem[m];
    p.layer[s] = layer[m];
    p.status[s] = sp.elem[m] > 0 ? FL_ACTIVE : FL_LEFT;
    p.fresh[s] = 1;
  }
  return 0;
}

// the host statement of one advance of the whole set on a state q_df(3,npoin,L) -- what the kernel runs
template <int NGL>
inline void float_advance_all_ngl(const FloatField &f, double dt, FloatPlan &p) {
  for (int64_t s = 0; s < p.M; s++) {
    FloatRec r;
    p.get((size_t)s, r);
    float_advance<NGL>(f, dt, r, FloatVelPlain{});
    p.put((size_t)s, r);
  }
}

inline FloatField float_field(const FloatGeom &g, const double *q, size_t npoin) {
  FloatField f{};
  f.corners = g.corners.data();
  f.tol = g.tol.data();
  f.nbr = g.nbr.data();
  f.q = q;
  f.npoin = npoin;
  for (int i = 0; i < g.ngl && i < 8; i++) f.xgl[i] = g.xgl[i];
  return f;
}

inline void float_advance_all(const FloatGeom &g, const double *q, size_t npoin, double dt, FloatPlan &p) {
  const FloatField f = float_field(g, q, npoin);
  switch (g.ngl) {
    case 3: float_advance_all_ngl<3>(f, dt, p); break;
    case 4: float_advance_all_ngl<4>(f, dt, p); break;
    case 5: float_advance_all_ngl<5>(f, dt, p); break;
    case 6: float_advance_all_ngl<6>(f, dt, p); break;
    default: float_advance_all_ngl<8>(f, dt, p); break;
  }
}

// ------------------------------------------------------------------ migration, the host part
// The side table xface [nelem_owned][4][2] and the arrival table [sum num_send_recv] of a processor-face rank,
// from the halo lists (num_nbh neighbours, num_send_recv[k] 1-based local faces each in nbh_send_recv, in the
// order both ranks agree on): the side of face(7) that listed face `pos` of neighbour k lies on gets (k, pos),
// every other side (-1, -1); arrive[off_k + pos] = that element, 0-based.
inline int float_xface(const int32_t *face, const int32_t *imapl, int nface, int ngl, int nelem_owned, const std::vector<int32_t> &nbr,
                       int num_nbh, const int32_t *num_send_recv, const int32_t *nbh_send_recv, std::vector<int32_t> &xface,
                       std::vector<int32_t> &arrive, std::string &err) {
  const char *who = "hnumo_floats_migrate";
  if (!face || !imapl) return err = std::string(who) + ": face or imapl is NULL", SP_ERR_INVALID;
  if (num_nbh < 0 || (num_nbh > 0 && (!num_send_recv || !nbh_send_recv)))
    return err = std::string(who) + ": num_nbh < 0, or num_send_recv or nbh_send_recv is NULL", SP_ERR_INVALID;
  if (nelem_owned < 0 || nbr.size() != 4 * (size_t)nelem_owned)
    return err = std::string(who) + ": the side neighbours do not cover the owned elements", SP_ERR_INVALID;
  xface.assign(8 * (size_t)nelem_owned, -1);
  arrive.clear();
  size_t o = 0;
  for (int k = 0; k < num_nbh; k++) {
    if (num_send_recv[k] < 0) return err = std::string(who) + ": num_send_recv(" + std::to_string(k + 1) + ") < 0", SP_ERR_INVALID;
    for (int pos = 0; pos < num_send_recv[k]; pos++, o++) {
      const int f = nbh_send_recv[o] - 1;
      const std::string which = "face " + std::to_string(f + 1) + " (neighbour " + std::to_string(k + 1) + ", position " +
                                std::to_string(pos + 1) + ")";
      if (f < 0 || f >= nface) return err = std::string(who) + ": " + which + " is out of range", SP_ERR_INVALID;
      const int32_t el = face[8 * (size_t)f + 6];
      if (face[8 * (size_t)f + 7] != 0 || el < 1 || el > nelem_owned)
        return err = std::string(who) + ": " + which + " is not a processor face (face(8) = 0) of an owned element", SP_ERR_INVALID;
      const int sd = float_face_side(imapl, ngl, f);
      if (sd < 0 || sd > 3) return err = std::string(who) + ": the nodes of " + which + " are not one side of its element", SP_ERR_INVALID;
      const size_t t = 4 * (size_t)(el - 1) + sd;
      if (xface[2 * t] >= 0) return err = std::string(who) + ": " + which + " lies on a side that is listed already", SP_ERR_INVALID;
      if (nbr[t] != FL_OFF_RANK) return err = std::string(who) + ": " + which + " lies on a side that is not off-rank", SP_ERR_INVALID;
      xface[2 * t] = k;
      xface[2 * t + 1] = pos;
      arrive.push_back(el - 1);
    }
  }
  return 0;
}

// iperm[input position] = the kernel's slot
inline std::vector<int32_t> float_inverse_perm(const std::vector<int32_t> &perm) {
  std::vector<int32_t> ip(perm.size());
  for (size_t s = 0; s < perm.size(); s++) ip[perm[s]] = (int32_t)s;
  return ip;
}

// what an arrival is checked for before it is run: values no sender produces would leave the hop loop unbounded
HNUMO_HD inline bool float_flight_ok(const FloatFlight &fl, int64_t M, int nlayers, int nfaces) {
  return fl.gid >= 0 && fl.gid < M && fl.layer >= 1 && fl.layer <= nlayers && (fl.stage == 0 || fl.stage == 1) && fl.hops >= 1 &&
         fl.hops <= FL_MAXHOPS && fl.pos >= 0 && fl.pos < nfaces;
}

// a rank's side of a migrating set on the host: what the kernels read
struct FloatRank {
  const FloatGeom *g = nullptr;
  std::vector<double> tol;               // tol_e under the set's coord_scale (g->tol without one)
  std::vector<int32_t> xface, arrive, iperm;
  std::vector<int> off, cnt;             // per neighbour: its segment of arrive
  FloatField field(const double *q, size_t npoin) const {
    FloatField f = float_field(*g, q, npoin);
    f.tol = tol.data();
    return f;
  }
};

// the host statement of float_advance_kernel<NGL, 1, true>: one advance of the whole set, flights appended to out
template <int NGL>
inline void float_advance_mig_ngl(const FloatRank &rk, const FloatField &f, double dt, FloatPlan &p, std::vector<FloatFlight> &out) {
  for (int64_t s = 0; s < p.M; s++) {
    FloatRec r;
    p.get((size_t)s, r);
    FloatFlight fl{};
    if (float_advance<NGL, true>(f, dt, r, FloatVelPlain{}, rk.xface.data(), &fl)) {
      fl.gid = p.perm[s];
      out.push_back(fl);
    }
    p.put((size_t)s, r);
  }
}

// the host statement of float_arrive_kernel<NGL>: the entries of a sender's outbox addressed to neighbour index
// want_k of the sender, which is this rank's neighbour `from`
template <int NGL>
inline void float_arrive_ngl(const FloatRank &rk, const FloatField &f, int nlayers, const std::vector<FloatFlight> &in, int want_k,
                             int from, FloatPlan &p, std::vector<FloatFlight> &out) {
  for (const FloatFlight &a : in) {
    if (a.k != want_k || !float_flight_ok(a, p.M, nlayers, rk.cnt[from])) continue;
    const size_t s = (size_t)rk.iperm[a.gid];
    FloatRec r;
    p.get(s, r);
    FloatFlight fl{};
    if (float_resume<NGL>(f, rk.xface.data(), a, rk.arrive[rk.off[from] + a.pos], r, FloatVelPlain{}, &fl)) {
      fl.gid = a.gid;
      out.push_back(fl);
    }
    p.put(s, r);
  }
}

// ------------------------------------------------------------------ sensors (include/hnumo_engine.h has the normative text)
// A set's sensor mask adds S rows to a record: STATE (1) h, u, v, dp, elevation and VORT (2) zeta, delta, pv, ow of
// the float's own layer, each the value a hnumo_sample_create_ref set reads at the float's cached (elem, xi, eta).
// float_sense_kernel (kernels_float.hip) and float_sense_host below run the same text: the slot rule
// (float_sense_slots is its sequential statement; the kernel forms it with a ballot), the forming of an element's
// nodal fields into an arena of K element slots with an odd stride, and the double sum.  The forming statements
// restate diag_layer_fields (kernels_diag.hip) and vort_node (kernels_vort.hip), which sample_kernel is compiled
// from and which stay as they are.
constexpr int FL_SENSE_STATE = 1, FL_SENSE_VORT = 2;   // HNUMO_FLOAT_SENSE_STATE, HNUMO_FLOAT_SENSE_VORT
constexpr int FL_SENSE_ALL = FL_SENSE_STATE | FL_SENSE_VORT;
constexpr int FL_SENSE_LDS_BYTES = 32768;              // the kernel's arena

// rows per float, rows per element in the arena (every layer: the floats of an element lie in any), the arena's
// element stride in doubles (odd: consecutive slots start on different LDS banks) and its element slots K
constexpr int fl_sense_rows(int mask) { return (mask & FL_SENSE_STATE ? 5 : 0) + (mask & FL_SENSE_VORT ? 4 : 0); }
constexpr int fl_sense_nval(int L, int mask) { return fl_sense_rows(mask) * L; }
constexpr int fl_sense_estride(int ngl, int L, int mask) { return (fl_sense_nval(L, mask) * ngl * ngl) | 1; }
constexpr int fl_sense_K(int ngl, int L, int mask) {
  return mask ? FL_SENSE_LDS_BYTES / (8 * fl_sense_estride(ngl, L, mask)) : 0;
}

// what the sensors read beside the floats: the state, the statics of diag_layer_fields and of vort_node
struct FloatSense {
  const double *q;                  // q_df(3, npoin, L)
  const double *zbot, *alpha;       // zbot_df(npoin), alpha_mlswe(L)
  const double *ex, *ey, *nx, *ny;  // ksi_x, ksi_y, eta_x, eta_y (npoin)
  const double *f;                  // coriolis_df(npoin) as hnumo_vort_begin took it, or NULL: 0
  const double *dpsi;               // D(m,i) at [m*ngl + i]
  double gravity;
  size_t npoin;
  double xgl[8];
};

// The slot rule for n consecutive floats of a set (one workgroup's; elem 1-based, <= 0: inactive): a float is a
// head when it is active and it is the first, or the float before it is inactive or lies in another element; the
// slot of an active float is the inclusive count of heads up to it, minus 1 (-1 for an inactive one); list[slot] =
// the head's element, 0-based.  Returns the number of slots.  An element that turns up in two separate runs gets
// two slots.
inline int float_sense_slots(const int32_t *elem, int n, int32_t *slot, int32_t *list) {
  int ns = 0;
  for (int t = 0; t < n; t++) {
    if (elem[t] <= 0) {
      slot[t] = -1;
      continue;
    }
    if (t == 0 || elem[t - 1] <= 0 || elem[t - 1] != elem[t]) list[ns++] = elem[t] - 1;
    slot[t] = ns - 1;
  }
  return ns;
}

// STATE: the rows 5k..5k+4 = h, u, v, dp, elevation of node I into s[(5k + v) * P] (diag_layer_fields' statements)
template <int NGL, int L>
HNUMO_HD inline void float_sense_form_state(const FloatSense &g, const double (&ag)[L], size_t I, double *s) {
  constexpr int P = NGL * NGL;
  double f[L][5];
#pragma unroll
  for (int k = 0; k < L; k++) {
    const double *p = g.q + 3 * (I + g.npoin * k);
    const double dp = p[0];
    f[k][0] = ag[k] * dp;
    f[k][1] = p[1] / dp;
    f[k][2] = p[2] / dp;
    f[k][3] = dp;
  }
  double elev = g.zbot[I];
#pragma unroll
  for (int k = L - 1; k >= 0; k--) {
    elev = elev + f[k][0];
    f[k][4] = elev;
  }
#pragma unroll
  for (int k = 0; k < L; k++)
#pragma unroll
    for (int v = 0; v < 5; v++) s[(5 * k + v) * P] = f[k][v];
}

// VORT, the three steps of sample_kernel's VORT source for node I = (i, j) of an element whose rows start at se,
// s = se + j*NGL + i.  1: u, v of every layer into rows 4k+2, 4k+3, h kept.  (All nodes of the element, then) 2: zeta,
// delta into rows 4k, 4k+1, pv and ow kept (vort_node's statements).  (All nodes, then) 3: pv, ow into rows 4k+2, 4k+3.
template <int NGL, int L>
HNUMO_HD inline void float_sense_vort_uv(const FloatSense &g, const double (&ag)[L], size_t I, double *s, double (&h)[L]) {
  constexpr int P = NGL * NGL;
#pragma unroll
  for (int k = 0; k < L; k++) {
    const double *p = g.q + 3 * (I + g.npoin * k);
    const double dp = p[0];
    h[k] = ag[k] * dp;
    s[(4 * k + 2) * P] = p[1] / dp;
    s[(4 * k + 3) * P] = p[2] / dp;
  }
}

template <int NGL, int L>
HNUMO_HD inline void float_sense_vort_node(const FloatSense &g, size_t I, int i, int j, const double *se, double *s,
                                           const double (&h)[L], double (&pvow)[L][2]) {
  constexpr int P = NGL * NGL;
  double Di[NGL], Dj[NGL];
#pragma unroll
  for (int m = 0; m < NGL; m++) {
    Di[m] = g.dpsi[m * NGL + i];
    Dj[m] = g.dpsi[m * NGL + j];
  }
  const double ex = g.ex[I], ey = g.ey[I], nx = g.nx[I], ny = g.ny[I];
  const double f = g.f ? g.f[I] : 0.0;
#pragma unroll
  for (int k = 0; k < L; k++) {
    const double *su = se + (4 * k + 2) * P, *sv = se + (4 * k + 3) * P;
    const double *ur = su + j * NGL, *vr = sv + j * NGL, *uc = su + i, *vc = sv + i;
    double u_xi = Di[0] * ur[0], u_eta = Dj[0] * uc[0], v_xi = Di[0] * vr[0], v_eta = Dj[0] * vc[0];
#pragma unroll
    for (int m = 1; m < NGL; m++) {
      u_xi = u_xi + Di[m] * ur[m];
      u_eta = u_eta + Dj[m] * uc[m * NGL];
      v_xi = v_xi + Di[m] * vr[m];
      v_eta = v_eta + Dj[m] * vc[m * NGL];
    }
    const double u_x = u_xi * ex + u_eta * nx, u_y = u_xi * ey + u_eta * ny;
    const double v_x = v_xi * ex + v_eta * nx, v_y = v_xi * ey + v_eta * ny;
    const double zeta = v_x - u_y;
    const double sn = u_x - v_y, ss = v_x + u_y;
    s[(4 * k) * P] = zeta;
    s[(4 * k + 1) * P] = u_x + v_y;
    pvow[k][0] = (zeta + f) / h[k];
    pvow[k][1] = (sn * sn + ss * ss) - zeta * zeta;
  }
}

template <int NGL, int L>
HNUMO_HD inline void float_sense_vort_store(double *s, const double (&pvow)[L][2]) {
  constexpr int P = NGL * NGL;
#pragma unroll
  for (int k = 0; k < L; k++) {
    s[(4 * k + 2) * P] = pvow[k][0];
    s[(4 * k + 3) * P] = pvow[k][1];
  }
}

// a float's 2 NGL weights (float_vel's statement) and one row of its value from the tile f[j*NGL + i]
template <int NGL>
HNUMO_HD inline void float_sense_weights(const double *xgl, double xi, double eta, double (&lx)[NGL], double (&ly)[NGL]) {
#pragma unroll
  for (int i = 0; i < NGL; i++) {
    double wx = 1.0, wy = 1.0;
#pragma unroll
    for (int m = 0; m < NGL; m++)
      if (m != i) {
        wx = wx * ((xi - xgl[m]) / (xgl[i] - xgl[m]));
        wy = wy * ((eta - xgl[m]) / (xgl[i] - xgl[m]));
      }
    lx[i] = wx;
    ly[i] = wy;
  }
}

template <int NGL>
HNUMO_HD inline double float_sense_value(const double *f, const double (&lx)[NGL], const double (&ly)[NGL]) {
  double val = 0.0;
#pragma unroll
  for (int j = 0; j < NGL; j++) {
    double r = lx[0] * f[j * NGL];
#pragma unroll
    for (int i = 1; i < NGL; i++) r = r + lx[i] * f[j * NGL + i];
    val = j == 0 ? ly[0] * r : val + ly[j] * r;
  }
  return val;
}

// the S rows of a float of layer k (0-based) whose element's rows start at se, into o[row * stride]
template <int NGL, int L, int MASK>
HNUMO_HD inline void float_sense_rows_of(const double *se, int k, const double (&lx)[NGL], const double (&ly)[NGL], double *o,
                                         size_t stride) {
  constexpr int P = NGL * NGL, VO = MASK & FL_SENSE_STATE ? 5 * L : 0;
  int row = 0;
  if constexpr ((MASK & FL_SENSE_STATE) != 0) {
#pragma unroll
    for (int v = 0; v < 5; v++) o[(size_t)(row++) * stride] = float_sense_value<NGL>(se + (5 * k + v) * P, lx, ly);
  }
  if constexpr ((MASK & FL_SENSE_VORT) != 0) {
#pragma unroll
    for (int v = 0; v < 4; v++) o[(size_t)(row++) * stride] = float_sense_value<NGL>(se + (VO + 4 * k + v) * P, lx, ly);
  }
}

// The host statement of float_sense_kernel<NGL, L, MASK>: out [S][M] planar, in input order; K: the element slots
// of a pass (the kernel's fl_sense_K; any K >= 1 gives the same bits).
template <int NGL, int L, int MASK>
inline void float_sense_host_t(const FloatSense &g, const FloatPlan &p, int K, double *out) {
  constexpr int P = NGL * NGL, S = fl_sense_rows(MASK), ES = fl_sense_estride(NGL, L, MASK), VO = MASK & FL_SENSE_STATE ? 5 * L : 0;
  const size_t M = (size_t)p.M;
  std::vector<double> arena((size_t)K * ES);
  double ag[L];
  for (int k = 0; k < L; k++) ag[k] = g.alpha[k] / g.gravity;
  for (size_t b0 = 0; b0 < M; b0 += FL_BLOCK) {
    const int n = (int)std::min<size_t>(FL_BLOCK, M - b0);
    int32_t slot[FL_BLOCK], list[FL_BLOCK];
    const int nslots = float_sense_slots(p.elem.data() + b0, n, slot, list);
    for (int p0 = 0; p0 < nslots; p0 += K) {
      const int nel = std::min(K, nslots - p0);
      for (int le = 0; le < nel; le++) {
        double *se = arena.data() + (size_t)le * ES;
        const size_t I0 = (size_t)list[p0 + le] * P;
        if constexpr ((MASK & FL_SENSE_STATE) != 0)
          for (int ln = 0; ln < P; ln++) float_sense_form_state<NGL, L>(g, ag, I0 + ln, se + ln);
        if constexpr ((MASK & FL_SENSE_VORT) != 0) {
          double h[P][L], pvow[P][L][2];
          for (int ln = 0; ln < P; ln++) float_sense_vort_uv<NGL, L>(g, ag, I0 + ln, se + VO * P + ln, h[ln]);
          for (int ln = 0; ln < P; ln++)
            float_sense_vort_node<NGL, L>(g, I0 + ln, ln % NGL, ln / NGL, se + VO * P, se + VO * P + ln, h[ln], pvow[ln]);
          for (int ln = 0; ln < P; ln++) float_sense_vort_store<NGL, L>(se + VO * P + ln, pvow[ln]);
        }
      }
      for (int t = 0; t < n; t++) {
        if (slot[t] < p0 || slot[t] >= p0 + nel) continue;
        const size_t s = b0 + t;
        double lx[NGL], ly[NGL];
        float_sense_weights<NGL>(g.xgl, p.xi[s], p.eta[s], lx, ly);
        float_sense_rows_of<NGL, L, MASK>(arena.data() + (size_t)(slot[t] - p0) * ES, p.layer[s] - 1, lx, ly, out + p.perm[s], M);
      }
    }
    for (int t = 0; t < n; t++)
      if (slot[t] < 0)
        for (int v = 0; v < S; v++) out[(size_t)v * M + p.perm[b0 + t]] = 0.0;
  }
}

template <class F>
inline void float_with_ngl(int ngl, F &&fn) {
  switch (ngl) {
    case 3: fn(std::integral_constant<int, 3>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    case 5: fn(std::integral_constant<int, 5>{}); break;
    case 6: fn(std::integral_constant<int, 6>{}); break;
    default: fn(std::integral_constant<int, 8>{}); break;
  }
}

// fn(integral_constant L, integral_constant MASK) for L in 1..3 and a mask in 1..3
template <class F>
inline void float_with_L_mask(int L, int mask, F &&fn) {
  auto with_mask = [&](auto l) {
    switch (mask) {
      case FL_SENSE_STATE: fn(l, std::integral_constant<int, FL_SENSE_STATE>{}); break;
      case FL_SENSE_VORT: fn(l, std::integral_constant<int, FL_SENSE_VORT>{}); break;
      default: fn(l, std::integral_constant<int, FL_SENSE_ALL>{}); break;
    }
  };
  switch (L) {
    case 1: with_mask(std::integral_constant<int, 1>{}); break;
    case 2: with_mask(std::integral_constant<int, 2>{}); break;
    default: with_mask(std::integral_constant<int, 3>{}); break;
  }
}

// the sensors of the whole set on the host, in passes of K element slots (K <= 0: the kernel's)
inline void float_sense_host(int ngl, int L, int mask, const FloatSense &g, const FloatPlan &p, int K, double *out) {
  float_with_ngl(ngl, [&](auto n) {
    float_with_L_mask(L, mask, [&](auto l, auto m) {
      constexpr int NGL = decltype(n)::value, LL = decltype(l)::value, MASK = decltype(m)::value;
      float_sense_host_t<NGL, LL, MASK>(g, p, K > 0 ? K : fl_sense_K(NGL, LL, MASK), out);
    });
  });
}

}  // namespace hnumo
