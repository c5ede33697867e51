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
// few elements.  No atomics (but the migrating sets' one integer add per wave, below), nothing between
// workgroups, no LDS; every loop over registers has compile-time bounds, the Newton and hop loops are
// bounded by 32 and 4.
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
// positions; float_sense_kernel<NGL, L, MASK> (at the end of this file, the one kernel here with LDS)
// appends the S rows of the set's sensors behind it.
//
// Migrating sets (processor-face ranks): float_advance_kernel<NGL, 1, true> is the same advance with
// float_plan.h's MIG flag: a lane whose float reaches a processor face appends its flight record to the
// rank's outbox -- SoA, 7 double and 6 int32 planes of capacity M -- by one integer atomicAdd per wave
// (ballot, lanes ranked by the ballot prefix).  The order of an outbox is not deterministic and nothing
// depends on it: float_arrive_kernel<NGL>, one lane per entry of a sender's outbox, drops the entries
// addressed to another rank, resumes the float in the element behind the face (float_resume) and stores
// it in its own slot iperm[gid]; a float that goes into flight again is appended to the receiver's outbox
// of the next round.  No LDS, no floating-point atomics.  <NGL, G, false> is the kernel as it was.
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

// an outbox: planes [FL_FD][cap] (x, y, wx, wy, dt, px, py) and [FL_FI][cap] (gid, layer, stage, hops, k, pos)
struct FloatBox {
  double *d;
  int *i;
  int *count;
  size_t cap;
};

struct FloatMigArgs {
  FloatArgs a;
  const int *xface;                        // [E][4][2]
  FloatBox out;
};

struct FloatArriveArgs {
  FloatArgs a;                             // the receiver's floats and field
  const int *xface, *arrive, *iperm;       // the receiver's tables; arrive at the sender's segment
  FloatBox in, out;                        // the sender's outbox of this round, the receiver's of the next
  int n;                                   // entries of `in` (the host has read the count)
  int want_k;                              // the k that addresses the receiver in `in`
  int nfaces, nlayers;                     // faces the two ranks share; layers
};

struct FloatMarkArgs {
  FloatArgs a;
  const int *gid, *iperm;
  int n, status;                           // status LEFT: release ACTIVE floats; LOST: whatever they are
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

// appends the flight records of the lanes with `go`: one atomicAdd per wave, lanes ranked by the ballot prefix
__device__ inline void float_box_append(const FloatBox &b, bool go, const FloatFlight &fl) {
  const unsigned long long m = __ballot(go);
  if (!go) return;
  const int lane = (int)__lane_id(), leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(b.count, __popcll(m));
  base = __shfl(base, leader);
  const size_t t = (size_t)base + (size_t)__popcll(m & ((1ull << lane) - 1ull));
  if (t >= b.cap) return;                  // (a float is in flight once: an outbox never holds more than M)
  const double d[FL_FD] = {fl.x, fl.y, fl.wx, fl.wy, fl.dt, fl.px, fl.py};
  const int i[FL_FI] = {fl.gid, fl.layer, fl.stage, fl.hops, fl.k, fl.pos};
#pragma unroll
  for (int v = 0; v < FL_FD; v++) b.d[v * b.cap + t] = d[v];
#pragma unroll
  for (int v = 0; v < FL_FI; v++) b.i[v * b.cap + t] = i[v];
}

__device__ inline void float_store(const FloatArgs &a, size_t s, const FloatRec &r) {
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

template <int NGL, int G, bool MIG>
__global__ void __launch_bounds__(FL_BLOCK) float_advance_kernel(std::conditional_t<MIG, FloatMigArgs, FloatArgs> arg) {
  if constexpr (MIG) {
    static_assert(G == 1, "migrating sets use the one-lane mapping");
    const FloatArgs &a = arg.a;
    const size_t s = (size_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    bool go = false;
    FloatFlight fl{};
    if (s < a.M && a.status[s] == FL_ACTIVE) {
      FloatRec r{a.x[s], a.y[s], a.wx[s], a.wy[s], a.xi[s], a.eta[s], a.elem[s], a.layer[s], FL_ACTIVE, a.fresh[s]};
      go = float_advance<NGL, true>(a.f, a.dt, r, FloatVelPlain{}, arg.xface, &fl);
      fl.gid = a.perm[s];
      float_store(a, s, r);
    }
    float_box_append(arg.out, go, fl);
  } else {
    static_assert(G == 1 || (G >= NGL && FL_BLOCK % G == 0 && 64 % G == 0), "a float's lanes lie in one wave");
    const FloatArgs &a = arg;
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
    float_store(a, s, r);
  }
}

template <int NGL>
__global__ void __launch_bounds__(FL_BLOCK) float_arrive_kernel(FloatArriveArgs g) {
  const FloatArgs &a = g.a;
  const size_t t = (size_t)blockIdx.x * FL_BLOCK + threadIdx.x;
  bool go = false;
  FloatFlight fl{};
  if (t < (size_t)g.n && g.in.i[4 * g.in.cap + t] == g.want_k) {
    const double *d = g.in.d + t;
    const int *i = g.in.i + t;
    const size_t c = g.in.cap;
    const FloatFlight in{d[0], d[c], d[2 * c], d[3 * c], d[4 * c], d[5 * c], d[6 * c], i[0], i[c], i[2 * c], i[3 * c], i[4 * c], i[5 * c]};
    if (float_flight_ok(in, (int64_t)a.M, g.nlayers, g.nfaces)) {
      const size_t s = (size_t)g.iperm[in.gid];
      FloatRec r{a.x[s], a.y[s], a.wx[s], a.wy[s], a.xi[s], a.eta[s], a.elem[s], in.layer, FL_ACTIVE, 0};
      go = float_resume<NGL>(a.f, g.xface, in, g.arrive[in.pos], r, FloatVelPlain{}, &fl);
      fl.gid = in.gid;
      float_store(a, s, r);
    }
  }
  float_box_append(g.out, go, fl);
}

// the floats gid[0..n) of the input become `status` with elem 0, w 0 where they are: LEFT releases the ACTIVE ones
// (a seed that another rank keeps), LOST is for a float still in flight after the last round
__global__ void __launch_bounds__(FL_BLOCK) float_mark_kernel(FloatMarkArgs g) {
  const size_t t = (size_t)blockIdx.x * FL_BLOCK + threadIdx.x;
  if (t >= (size_t)g.n) return;
  const int m = g.gid[t];
  if (m < 0 || (size_t)m >= g.a.M) return;
  const size_t s = (size_t)g.iperm[m];
  if (g.status == FL_LEFT && g.a.status[s] != FL_ACTIVE) return;
  g.a.status[s] = g.status;
  g.a.elem[s] = 0;
  g.a.wx[s] = g.a.wy[s] = 0.0;
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

// float_sense_kernel<NGL, L, MASK>: the sensor rows of a record (float_plan.h has the statements, which its host
// evaluation float_sense_host_t runs too).  One workgroup per FL_BLOCK consecutive slots of the set's sorted order.
//   Slots: a lane is a head when its float is active (elem > 0) and it is lane 0 or the float before it is inactive
//   or in another element; a wave counts its heads with a ballot, the lane's inclusive count is the popcount of the
//   ballot up to its own bit, the four waves' totals go through LDS; heads publish their element in s_list.
//   Passes of K slots (the trip count ceil(nslots / K) is the workgroup's, so every lane reaches every barrier):
//   the nodal fields of the pass's elements go into the arena of K * ES doubles (ES odd) -- STATE one node per lane
//   in a strided loop, VORT in passes of 256/P whole elements with sample_kernel's u, v -> barrier -> derivative
//   sums -> barrier -> pv, ow sequence; consecutive lanes read consecutive nodes of q.  One barrier.  A lane whose
//   slot lies in the pass forms its 2 NGL weights in registers, evaluates its S rows of its own layer (lanes of one
//   element read the same words: broadcasts) and writes out[row][perm[s]].  One barrier before the next pass.
//   Inactive floats write S zeros.
// No atomics, nothing between workgroups; every loop over registers has compile-time bounds; a value is one lane's
// sum, so the grouping (and an element that takes two slots) cannot change a bit.
struct FloatSenseArgs {
  FloatSense g;
  const double *xi, *eta;
  const int *elem, *layer, *perm;
  double *out;                             // [S][M]
  size_t M;
};

template <int NGL, int L, int MASK>
__global__ void __launch_bounds__(FL_BLOCK) float_sense_kernel(FloatSenseArgs a) {
  constexpr int P = NGL * NGL, S = fl_sense_rows(MASK), ES = fl_sense_estride(NGL, L, MASK), K = fl_sense_K(NGL, L, MASK);
  constexpr int VO = MASK & FL_SENSE_STATE ? 5 * L : 0, NW = FL_BLOCK / 64;
  static_assert(K >= 1, "the arena holds no element");
  static_assert(FL_BLOCK % 64 == 0, "whole waves");
  __shared__ double s_f[K * ES];
  __shared__ int s_list[FL_BLOCK];
  __shared__ int s_heads[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t s = (size_t)blockIdx.x * FL_BLOCK + tid;
  const bool in = s < a.M;
  const int e = in ? a.elem[s] : 0;
  const bool active = e > 0;
  const int before = (in && tid > 0) ? a.elem[s - 1] : 0;
  const bool head = active && (tid == 0 || before <= 0 || before != e);
  const unsigned long long heads = __ballot(head);
  if (lane == 0) s_heads[wave] = __popcll(heads);
  __syncthreads();
  int base = 0, nslots = 0;
#pragma unroll
  for (int w = 0; w < NW; w++) {
    const int c = s_heads[w];
    base += w < wave ? c : 0;
    nslots += c;
  }
  const int slot = active ? base + __popcll(heads & (~0ull >> (63 - lane))) - 1 : -1;
  if (head) s_list[slot] = e - 1;
  __syncthreads();

  double ag[L];
#pragma unroll
  for (int k = 0; k < L; k++) ag[k] = a.g.alpha[k] / a.g.gravity;
  for (int p0 = 0; p0 < nslots; p0 += K) {       // (nslots is the workgroup's: every lane makes every pass)
    const int nel = nslots - p0 < K ? nslots - p0 : K;
    if constexpr ((MASK & FL_SENSE_STATE) != 0) {
      for (int t = tid; t < nel * P; t += FL_BLOCK) {
        const int le = t / P, ln = t - le * P;
        float_sense_form_state<NGL, L>(a.g, ag, (size_t)s_list[p0 + le] * P + ln, s_f + le * ES + ln);
      }
    }
    if constexpr ((MASK & FL_SENSE_VORT) != 0) {
      constexpr int EPI = FL_BLOCK / P;            // whole elements per pass
      const int le0 = tid / P, ln = tid - le0 * P, j = ln / NGL, i = ln - j * NGL;
      for (int b = 0; b < nel; b += EPI) {
        const int le = b + le0;
        const bool act = tid < EPI * P && le < nel;
        double *se = s_f + (act ? le : 0) * ES + VO * P;
        size_t I = 0;
        double h[L], pvow[L][2];
        if (act) {
          I = (size_t)s_list[p0 + le] * P + ln;
          float_sense_vort_uv<NGL, L>(a.g, ag, I, se + ln, h);
        }
        __syncthreads();
        if (act) float_sense_vort_node<NGL, L>(a.g, I, i, j, se, se + ln, h, pvow);
        __syncthreads();
        if (act) float_sense_vort_store<NGL, L>(se + ln, pvow);
      }
    }
    __syncthreads();
    if (active && slot >= p0 && slot < p0 + nel) {
      double lx[NGL], ly[NGL];
      float_sense_weights<NGL>(a.g.xgl, a.xi[s], a.eta[s], lx, ly);
      float_sense_rows_of<NGL, L, MASK>(s_f + (slot - p0) * ES, a.layer[s] - 1, lx, ly, a.out + a.perm[s], a.M);
    }
    __syncthreads();
  }
  if (in && !active) {
    double *o = a.out + a.perm[s];
#pragma unroll
    for (int v = 0; v < S; v++) o[(size_t)v * a.M] = 0.0;
  }
}

}  // namespace hnumo
