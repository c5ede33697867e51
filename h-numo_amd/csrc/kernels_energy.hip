// kernels_energy.hip -- the energy budget of the engine's device state: the power the wind puts into the
// top layer, the power the bottom drag removes, the interior viscous dissipation, and the kinetic and
// available potential energy these change.
//
// The first observer that works at the quadrature points, where the model applies its forcing: the layer
// state is interpolated from the LGL nodes to the element's quad points by sum factorisation in LDS,
// multiplied there with the resident wind (the QS_TW1/QS_TW2 rows wind_blend keeps current) and the drag
// law of mod_rhs_btp.F90:157-168, and integrated with the quad weights into a series.
//
// Definitions (normative; include/hnumo_engine.h, energy_plan.h; IEEE double, built with
// -ffp-contract=off: no FMA; every sum left to right from its first product).  Owned element e, nodes
// I = e*P + j*ngl + i, quad points Iq = e*Q + jq*nq + iq (nq = 2*ngl - 1), w_I the nodal jac, wq_Iq the quad
// weight wjac (QS_W), tau(1:2,Iq) the wind as it stands on the device at the time of the sample.  At the
// nodes, per layer k:
//
//   dp = q(1,I,k);  u = q(2,I,k)/dp;  v = q(3,I,k)/dp;  m = dp/gravity            (mass per area)
//   ke_k  = (0.5*(u*u + v*v))*m
//   z_k   = elevation of layer k's top interface as hnumo_layer_fields forms it (row 5)
//   d_k   = z_k - zref(I,k)                                   (zref given at begin; NULL: 0.0)
//   c_1   = 0.5*(gravity*(1.0/alpha_1));  c_k = 0.5*(gravity*(1.0/alpha_k - 1.0/alpha_(k-1)))  (k >= 2)
//   ape_k = c_k*(d_k*d_k)
//   u_x,u_y,v_x,v_y = the element's own gradient, the statements of vort_node (kernels_vort.hip), unchanged
//   eps_k = (visc_mlswe*((u_x*u_x + u_y*u_y) + (v_x*v_x + v_y*v_y)))*m
//
// At the quad points, node->quad interpolation of a nodal field a(i,j) in two passes in this order:
//
//   t(iq,n)  = psiq(1,iq)*a(1,n);  for m = 2..ngl: t = t + psiq(m,iq)*a(m,n)
//   A(iq,jq) = psiq(1,jq)*t(iq,1); for n = 2..ngl: A = A + psiq(n,jq)*t(iq,n)
//
// applied to u_1, v_1 (top layer) and u_L, v_L, dp_L (bottom layer): U1, V1, UL, VL, DPL.  Then
//
//   W = tau(1,Iq)*U1 + tau(2,Iq)*V1
//   botfr == 0:  D = +0.0                                         (nothing interpolated for it)
//   botfr == 1:  spd = (cd_mlswe/gravity)*DPL
//   botfr == 2:  spd = (cd_mlswe/alpha_L)*sqrt(UL*UL + VL*VL)
//                tb_u = spd*UL;  tb_v = spd*VL;  D = tb_u*UL + tb_v*VL
//
// One SAMPLE adds W, D to S_W, S_D per quad point (one double2 per quad point) and eps_k to S_V per node and
// layer: plain adds in sample order from +0.0, one lane owns a sum.  With a series it also forms the 3L+2
// integrals KE_1..L, APE_1..L, V_1..L, W, D over the rank's owned elements: nodal rows the products w_I*x_I
// added in node order per element, quad rows wq_Iq*x_Iq in quad order, from the first one; the element sums
// by the position-defined pairwise tree (stats_tree_kernel).  No floating-point atomics; plain vector loads
// and stores.  Ghost elements are never visited and read 0.  The host mirror is hnumo/energy.py
// (HostEnergy) and energy_plan.h's energy_host, equal bit for bit.
//
// What the terms are not: the drag law is evaluated on the layer state q, not on the sub-cycle's
// (qb, qprime) split or its time average; the wind is credited to the top layer; eps is the interior
// estimate, without the LDG face terms; the KE<->APE conversion is not formed.  The budget
// d(sum KE + sum APE)/dt ~ W - D - sum V closes to discretisation error, not to bits.
#include "energy_plan.h"
#include "engine_internal.h"

namespace hnumo {

struct EnergyArgs {
  const double *q;       // q_df(3,npoin,L)
  const double *alpha;   // alpha_mlswe(L)
  const double *nstat;   // nodal statics [NS_N][npoin]: the metric rows, NS_W (jac), NS_ZB (zbot_df)
  const double *qstat;   // quad statics [QS_N][npoin_q]: QS_W (wjac), QS_TW1, QS_TW2 (the resident wind)
  const double *zref;    // zref(npoin,L), or NULL: 0
  const double *psiq;    // psiq(m,iq) at [m*nq + iq]
  const double *dpsi;    // D(m,i) at [m*ngl + i]
  double2 *sq;           // (S_W, S_D) [npoin_q]
  double *sv;            // S_V [L][npoin]
  double *part;          // element partials [3L+2][ne] (SERIES)
  double gravity, cd, visc;
  int npoin, npq, ne;    // ne: the owned elements
};

// One sample.  A workgroup visits groups of EPG = 256/Q whole elements (the last group ragged); a lane is,
// by its number alone, the node tid of the group (tid < EPG*P), the entry tid of the first pass
// (tid < EPG*nq*ngl: element, n, iq with iq fastest) and the quad point tid (tid < EPG*Q: element, jq, iq),
// so its 2 ngl entries of D and 2 ngl entries of psiq sit in registers, loaded once per workgroup.
//   1  node lanes: load q, form u, v, dp, m; the u, v tiles of every layer and dp_L into LDS; ke, z, ape
//      (SERIES only: nothing else reads them).                                                 barrier
//   2  node lanes: vort_grad -> eps, read-modify-write of S_V.
//   3  first-pass lanes: t(iq,n) of the 2 (BOTFR = 0) or 5 fields into LDS.                    barrier
//   4  quad lanes: the second pass, W, D, the 16-byte read-modify-write of (S_W, S_D); SERIES: wq*W, wq*D
//      into LDS rows.                                                                          barrier
//   5  SERIES: one lane per (element, row) adds in order and writes the element partial.      barrier
// LDS banking (a ds_read_b64 is served per 32-lane half, bank = (addr/4) mod 64: two doubles conflict when
// their indices agree mod 32 and differ).  Pass 1 reads down the column n of the element's tile: the lanes
// of one n read one address (broadcast), the lanes of a half cover at most 32/nq + 2 consecutive columns of
// consecutive elements, ngl doubles apart in the unpadded tiles -- fewer than 32 doubles in all, no bank
// twice.  Pass 2 reads t at [e*TS + n*nq + iq]: the lanes of an element read nq consecutive doubles
// (different jq: the same address), a step of n moves all of them nq doubles.  Two elements in one half
// conflict when TS mod 32 lies within nq of 0: at ngl = 4 and 6 (28 and 66), where TS is padded by 16
// (en_tstride); tools/energy_banks.py enumerates every lane group of both passes and the pass 1 stores:
// conflict-free at every ngl.  The vort_grad reads are vort_kernel's (kernels_vort.hip).
template <int NGL, int L, int BOTFR, bool SERIES>
__global__ void __launch_bounds__(EN_BS) energy_sample_kernel(EnergyArgs a) {
  constexpr int NQ = 2 * NGL - 1, P = NGL * NGL, Q = NQ * NQ, EPG = EN_BS / Q, T1 = NQ * NGL, TS = en_tstride(NGL);
  constexpr int NF = BOTFR ? 5 : 2, R = en_rows(L);
  static_assert(EPG >= 1 && EPG * TS <= EN_BS, "one lane per first-pass entry");
  __shared__ double s_u[L][EPG * P], s_v[L][EPG * P], s_dp[BOTFR ? EPG * P : 1];
  __shared__ double s_t[NF][EPG * TS];
  __shared__ double s_pn[SERIES ? 3 * L : 1][SERIES ? EPG * P : 1], s_pq[SERIES ? 2 : 1][SERIES ? EPG * Q : 1];
  const int tid = threadIdx.x;
  const int le = tid / P, ln = tid - le * P, j = ln / NGL, i = ln - j * NGL;          // node lane
  const int e1 = tid / T1, r1 = tid - e1 * T1, n1 = r1 / NQ, iq1 = r1 - n1 * NQ;       // first-pass lane
  const int eq = tid / Q, rq = tid - eq * Q, jq = rq / NQ, iq = rq - jq * NQ;          // quad lane
  const int ngroups = (a.ne + EPG - 1) / EPG;
  const size_t npoin = (size_t)a.npoin, npq = (size_t)a.npq;
  double ag[L], ck[L], Di[NGL], Dj[NGL], ps1[NGL], ps2[NGL];
#pragma unroll
  for (int k = 0; k < L; k++) {
    ag[k] = a.alpha[k] / a.gravity;
    ck[k] = en_c(a.alpha, k, a.gravity);
  }
  const double alphaL = a.alpha[L - 1];
#pragma unroll
  for (int m = 0; m < NGL; m++) {
    Di[m] = a.dpsi[m * NGL + i];
    Dj[m] = a.dpsi[m * NGL + j];
    ps1[m] = a.psiq[m * NQ + iq1];
    ps2[m] = a.psiq[m * NQ + jq];
  }

  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int e0 = grp * EPG;
    const int nel = min(EPG, a.ne - e0);          // the last group may be ragged
    const bool act = tid < nel * P;
    const size_t I = (size_t)e0 * P + tid;
    double mk[L], w = 0.0;
    if (act) {
      double h[L];
      if (SERIES) w = a.nstat[(size_t)NS_W * npoin + I];
#pragma unroll
      for (int k = 0; k < L; k++) {
        double dp, u, v;
        en_node(a.q + 3 * (I + npoin * k), a.gravity, dp, u, v, mk[k]);
        h[k] = ag[k] * dp;
        s_u[k][tid] = u;
        s_v[k][tid] = v;
        if (BOTFR && k == L - 1) s_dp[tid] = dp;
        if (SERIES) s_pn[k][tid] = w * en_ke(u, v, mk[k]);
      }
      if (SERIES) {
        double z[L];
        double elev = a.nstat[(size_t)NS_ZB * npoin + I];
#pragma unroll
        for (int k = L - 1; k >= 0; k--) {
          elev = elev + h[k];
          z[k] = elev;
        }
#pragma unroll
        for (int k = 0; k < L; k++) s_pn[L + k][tid] = w * en_ape(ck[k], z[k], a.zref ? a.zref[I + npoin * k] : 0.0);
      }
    }
    __syncthreads();
    if (act) {
      const double ex = a.nstat[(size_t)NS_EX * npoin + I], ey = a.nstat[(size_t)NS_EY * npoin + I];
      const double nx = a.nstat[(size_t)NS_NX * npoin + I], ny = a.nstat[(size_t)NS_NY * npoin + I];
#pragma unroll
      for (int k = 0; k < L; k++) {
        double u_x, u_y, v_x, v_y;
        vort_grad<NGL>(s_u[k] + le * P, s_v[k] + le * P, i, j, Di, Dj, ex, ey, nx, ny, u_x, u_y, v_x, v_y);
        const double eps = en_eps(a.visc, u_x, u_y, v_x, v_y, mk[k]);
        double *s = a.sv + (size_t)k * npoin + I;
        *s = *s + eps;
        if (SERIES) s_pn[2 * L + k][tid] = w * eps;
      }
    }
    if (tid < nel * T1) {
      const int col = e1 * P + n1 * NGL, to = e1 * TS + r1;
      s_t[0][to] = en_dot<NGL>(ps1, s_u[0] + col, 1);
      s_t[1][to] = en_dot<NGL>(ps1, s_v[0] + col, 1);
      if constexpr (BOTFR != 0) {
        s_t[2][to] = en_dot<NGL>(ps1, s_u[L - 1] + col, 1);
        s_t[3][to] = en_dot<NGL>(ps1, s_v[L - 1] + col, 1);
        s_t[4][to] = en_dot<NGL>(ps1, s_dp + col, 1);
      }
    }
    __syncthreads();
    if (tid < nel * Q) {
      const size_t Iq = (size_t)e0 * Q + tid;
      const int to = eq * TS + iq;
      const double U1 = en_dot<NGL>(ps2, s_t[0] + to, NQ), V1 = en_dot<NGL>(ps2, s_t[1] + to, NQ);
      const double W = en_wind(a.qstat[(size_t)QS_TW1 * npq + Iq], a.qstat[(size_t)QS_TW2 * npq + Iq], U1, V1);
      double D = 0.0;
      if constexpr (BOTFR != 0) {
        const double UL = en_dot<NGL>(ps2, s_t[2] + to, NQ), VL = en_dot<NGL>(ps2, s_t[3] + to, NQ);
        const double DPL = en_dot<NGL>(ps2, s_t[4] + to, NQ);
        D = en_drag<BOTFR>(a.cd, a.gravity, alphaL, UL, VL, DPL);
      }
      double2 x = a.sq[Iq];
      x.x = x.x + W;
      x.y = x.y + D;
      a.sq[Iq] = x;
      if (SERIES) {
        const double wq = a.qstat[(size_t)QS_W * npq + Iq];
        s_pq[0][tid] = wq * W;
        s_pq[1][tid] = wq * D;
      }
    }
    __syncthreads();
    if (SERIES) {
      // lane -> (element of the group, row): the element index runs fastest
      for (int t = tid; t < nel * R; t += EN_BS) {
        const int el = t % nel, r = t / nel;
        const int n = r < 3 * L ? P : Q;
        const double *s = r < 3 * L ? s_pn[r] + el * P : s_pq[r - 3 * L] + el * Q;
        double sum = s[0];
        for (int x = 1; x < n; x++) sum = sum + s[x];
        a.part[(size_t)r * a.ne + e0 + el] = sum;
      }
      __syncthreads();
    }
  }
}

}  // namespace hnumo
