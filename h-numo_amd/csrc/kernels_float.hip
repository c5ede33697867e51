// kernels_float.hip -- Lagrangian floats advected through the resident state: a trajectory needs the
// velocity at the float's own position at every step, which the mlswe#### snapshots cannot give and
// a host pass pays a hnumo_sync per step for.
//
// The arithmetic is float_plan.h's float_vel / float_locate / float_advance, the text the CPU program
// of tests/test_float_plan.py runs; built with -ffp-contract=off: no FMA.  The numpy mirror is
// hnumo/floats.py (HostFloats), equal bit for bit.
//
// Floats are SoA in the set's sorted order (by initial element): x, y, wx, wy, xi, eta doubles and
// elem, layer, status, fresh int32, so a wave moves contiguous lines and its lanes start in the same
// few elements.  No atomics, nothing between workgroups, no LDS; every loop over registers has
// compile-time bounds, the Newton and hop loops are bounded by 32 and 4.
//
// float_advance_kernel<NGL, G>: G lanes per float.  G = 1 is the mapping in use; G > 1 was measured
// beside it (HNUMO_FLOAT_ROWS=1 with HNUMO_EXPERIMENTS=1) and is slower wherever the
// set fills the device: every lane of a group repeats the weights, the Newton iterations and their
// divisions, so G times the lanes do nearly G times the arithmetic to save loads that hit the cache.
//   G = 1  one lane does everything: an evaluation reads the element's 24 P bytes of the layer.
//   G > 1  (4 for NGL <= 4, 8 above) the G lanes of a float carry the same record and take the same
//          branches; in an evaluation lane j < NGL reads row j -- 24 NGL contiguous bytes -- and forms
//          r_j, the r_j go round by shuffles and every lane adds Ly[j] * r_j in order of j: each sum
//          is still one lane's, so the bits are those of G = 1.  Lane 0 of the group stores.
// float_record_kernel appends a record (x, y, u, v, elem) to the planar series at the floats' input
// positions.
#include "engine_internal.h"
#include "float_plan.h"

namespace hnumo {

struct FloatArgs {
  FloatField f;
  double *x, *y, *wx, *wy, *xi, *eta;
  int *elem, *status, *fresh;
  const int *layer, *perm;
  double *rec;                             // [FL_NREC][M] (float_record_kernel)
  double dt;
  size_t M;
};

constexpr int fl_group(int ngl) { return ngl <= 4 ? 4 : 8; }

// the G lanes of a float share an evaluation by rows
template <int G>
struct FloatVelRows {
  int g;                                   // this lane within its group
  template <int NGL>
  __device__ void eval(const FloatField &f, int k, int e, double xi, double eta, double &u, double &v) const {
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
    double ru = 0.0, rv = 0.0;
    if (g < NGL) {
      const double *r = f.q + 3 * ((size_t)e * (NGL * NGL) + f.npoin * (size_t)k) + 3 * g * NGL;
      ru = lx[0] * (r[1] / r[0]);
      rv = lx[0] * (r[2] / r[0]);
#pragma unroll
      for (int i = 1; i < NGL; i++) {
        ru = ru + lx[i] * (r[3 * i + 1] / r[3 * i]);
        rv = rv + lx[i] * (r[3 * i + 2] / r[3 * i]);
      }
    }
    u = v = 0.0;
#pragma unroll
    for (int j = 0; j < NGL; j++) {
      const double a = __shfl(ru, j, G), b = __shfl(rv, j, G);
      u = j == 0 ? ly[0] * a : u + ly[j] * a;
      v = j == 0 ? ly[0] * b : v + ly[j] * b;
    }
  }
};

template <int NGL, int G>
__global__ void __launch_bounds__(FL_BLOCK) float_advance_kernel(FloatArgs a) {
  static_assert(G == 1 || (G >= NGL && FL_BLOCK % G == 0 && 64 % G == 0), "a float's lanes lie in one wave");
  const size_t s = ((size_t)blockIdx.x * FL_BLOCK + threadIdx.x) / G;
  if (s >= a.M) return;
  if (a.status[s] != FL_ACTIVE) return;
  FloatRec r{a.x[s], a.y[s], a.wx[s], a.wy[s], a.xi[s], a.eta[s], a.elem[s], a.layer[s], FL_ACTIVE, a.fresh[s]};
  if constexpr (G == 1) {
    float_advance<NGL>(a.f, a.dt, r, FloatVelPlain{});
  } else {
    float_advance<NGL>(a.f, a.dt, r, FloatVelRows<G>{(int)(threadIdx.x % G)});
    if (threadIdx.x % G) return;
  }
  a.x[s] = r.x;
  a.y[s] = r.y;
  a.wx[s] = r.wx;
  a.wy[s] = r.wy;
  a.xi[s] = r.xi;
  a.eta[s] = r.eta;
  a.elem[s] = r.elem;
  a.status[s] = r.status;
  a.fresh[s] = r.fresh;
}

__global__ void __launch_bounds__(FL_BLOCK) float_record_kernel(FloatArgs a) {
  const size_t s = (size_t)blockIdx.x * FL_BLOCK + threadIdx.x;
  if (s >= a.M) return;
  double *o = a.rec + a.perm[s];
  o[0] = a.x[s];
  o[a.M] = a.y[s];
  o[2 * a.M] = a.wx[s];
  o[3 * a.M] = a.wy[s];
  o[4 * a.M] = (double)a.elem[s];
}

}  // namespace hnumo
