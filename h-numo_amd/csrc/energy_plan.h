// energy_plan.h -- the arithmetic of the energy budget (hnumo_energy_*, include/hnumo_engine.h), one text
// for energy_sample_kernel (kernels_energy.hip) and for the host loop energy_host below.  Plain C++17:
// no HIP, no engine; tests/energy_main.cpp compiles it with g++ and the sanitizers.
//
// Definitions (normative; include/hnumo_engine.h; IEEE double, no FMA, every sum left to
// right from its first product).  Owned element e, nodes I = e*P + j*ngl + i, quad points
// Iq = e*Q + jq*nq + iq (nq = 2*ngl - 1), w_I the nodal jac, wq_Iq the quad weight wjac, tau(1:2,Iq) the wind
// as it stands at the time of the sample.  At the nodes, per layer k:
//
//   dp = q(1,I,k);  u = q(2,I,k)/dp;  v = q(3,I,k)/dp;  m = dp/gravity            (mass per area)
//   ke_k  = (0.5*(u*u + v*v))*m
//   z_k   = elevation of layer k's top interface as hnumo_layer_fields forms it (row 5)
//   d_k   = z_k - zref(I,k)                                   (zref given at begin; NULL: 0.0)
//   c_1   = 0.5*(gravity*(1.0/alpha_1));  c_k = 0.5*(gravity*(1.0/alpha_k - 1.0/alpha_(k-1)))  (k >= 2)
//   ape_k = c_k*(d_k*d_k)
//   u_x,u_y,v_x,v_y = the element's own gradient, the statements of vort_node (kernels_vort.hip)
//   eps_k = (visc_mlswe*((u_x*u_x + u_y*u_y) + (v_x*v_x + v_y*v_y)))*m
//
// At the quad points a nodal field a(i,j) is interpolated in two passes, in this order:
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
// One sample adds W and D to S_W, S_D per quad point and eps_k to S_V per node and layer (plain adds in
// sample order from +0.0) and, with a series, forms the 3L+2 integrals KE_1..L, APE_1..L, V_1..L, W, D: per
// element the products w_I*x_I in node order (wq_Iq*x_Iq in quad order) from the first one, the element sums
// by the position-defined pairwise tree.  The kernel calls the functions below; the element gradient is
// vort_grad's there (kernels_vort.hip, the one device text of it) and restated in en_grad for the host loop,
// as float_plan.h restates it for the sensors.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#ifndef HNUMO_HD
#if defined(__HIPCC__)
#define HNUMO_HD __host__ __device__
#else
#define HNUMO_HD
#endif
#endif

namespace hnumo {

constexpr int EN_BS = 256;
constexpr int EN_MAXL = 3;
constexpr int en_rows(int L) { return 3 * L + 2; }
// elements per group of the 256-lane workgroup: whole elements, one lane per quad point
constexpr int en_epg(int ngl) { return EN_BS / ((2 * ngl - 1) * (2 * ngl - 1)); }
// element stride, in doubles, of the first pass' result t(iq,n) in LDS.  nq*ngl, plus 16 at ngl = 4 and 6:
// there a 32-lane half of the second pass that straddles two elements would meet the same banks at
// different addresses (28 and 66 are 28 and 2 mod 32, less than nq away from 0); 44 and 82 are 12 and 18
// mod 32, and a multiple of 16 keeps the first pass' stores of a 16-lane group on 16 banks
// (tools/energy_banks.py enumerates every lane group)
constexpr int en_tstride(int ngl) { return (2 * ngl - 1) * ngl + (ngl == 4 || ngl == 6 ? 16 : 0); }

// dp, u, v, m of a node from its three values of q
HNUMO_HD inline void en_node(const double *q3, double gravity, double &dp, double &u, double &v, double &m) {
  dp = q3[0];
  u = q3[1] / dp;
  v = q3[2] / dp;
  m = dp / gravity;
}

HNUMO_HD inline double en_ke(double u, double v, double m) { return (0.5 * (u * u + v * v)) * m; }

// c_k, k 0-based
HNUMO_HD inline double en_c(const double *alpha, int k, double gravity) {
  return k == 0 ? 0.5 * (gravity * (1.0 / alpha[0])) : 0.5 * (gravity * (1.0 / alpha[k] - 1.0 / alpha[k - 1]));
}

HNUMO_HD inline double en_ape(double c, double z, double zref) {
  const double d = z - zref;
  return c * (d * d);
}

HNUMO_HD inline double en_eps(double visc, double u_x, double u_y, double v_x, double v_y, double m) {
  return (visc * ((u_x * u_x + u_y * u_y) + (v_x * v_x + v_y * v_y))) * m;
}

// one entry of either pass: w[0]*x[0] + w[1]*x[stride] + ..., left to right
template <int NGL>
HNUMO_HD inline double en_dot(const double (&w)[NGL], const double *x, int stride) {
  double s = w[0] * x[0];
#pragma unroll
  for (int m = 1; m < NGL; m++) s = s + w[m] * x[m * stride];
  return s;
}

HNUMO_HD inline double en_wind(double t1, double t2, double U1, double V1) { return t1 * U1 + t2 * V1; }

// botfr 1 or 2 (botfr 0: D = +0.0, nothing is interpolated for it)
template <int BOTFR>
HNUMO_HD inline double en_drag(double cd, double gravity, double alphaL, double UL, double VL, double DPL) {
  const double spd = BOTFR == 1 ? (cd / gravity) * DPL : (cd / alphaL) * sqrt(UL * UL + VL * VL);
  const double tb_u = spd * UL, tb_v = spd * VL;
  return tb_u * UL + tb_v * VL;
}

// ------------------------------------------------------------------ the host loop
// the position-defined pairwise tree of the series (kernels_stats.hip: stats_tree_kernel)
inline double en_tree_sum(std::vector<double> x) {
  if (x.empty()) return 0.0;
  size_t n = x.size();
  while (n > 1) {
    const size_t h = (n + 1) / 2;
    for (size_t i = 0; i < h; i++) x[i] = 2 * i + 1 < n ? x[2 * i] + x[2 * i + 1] : x[2 * i];
    n = h;
  }
  return x[0];
}

struct EnergyHost {
  const double *q;                  // q_df(3,npoin,L)
  const double *alpha;              // alpha_mlswe(L)
  const double *zbot, *zref;        // zbot_df(npoin); zref(npoin,L) or NULL: 0.0
  const double *ex, *ey, *nx, *ny;  // ksi_x, ksi_y, eta_x, eta_y (npoin)
  const double *w, *wq;             // nodal jac (npoin), quad weight wjac (npoin_q)
  const double *tau;                // tau_wind(2,npoin_q)
  const double *dpsi, *psiq;        // D(m,i) at [m*ngl + i]; psiq(m,iq) at [m*nq + iq]
  double gravity, cd, visc;
  int botfr, L, ngl, ne;            // ne: the owned elements
  size_t npoin, npq;
};

// the element's own gradient at node (i, j): vort_node's statements (kernels_vort.hip), for the host
template <int NGL>
inline void en_grad(const double *su, const double *sv, int i, int j, const double *D, double ex, double ey, double nx,
                    double ny, double &u_x, double &u_y, double &v_x, double &v_y) {
  const double *ur = su + j * NGL, *vr = sv + j * NGL, *uc = su + i, *vc = sv + i;
  double u_xi = D[i] * ur[0], u_eta = D[j] * uc[0], v_xi = D[i] * vr[0], v_eta = D[j] * vc[0];
  for (int m = 1; m < NGL; m++) {
    u_xi = u_xi + D[m * NGL + i] * ur[m];
    u_eta = u_eta + D[m * NGL + j] * uc[m * NGL];
    v_xi = v_xi + D[m * NGL + i] * vr[m];
    v_eta = v_eta + D[m * NGL + j] * vc[m * NGL];
  }
  u_x = u_xi * ex + u_eta * nx, u_y = u_xi * ey + u_eta * ny;
  v_x = v_xi * ex + v_eta * nx, v_y = v_xi * ey + v_eta * ny;
}

// One sample of the state g.q, element by element in the kernel's phases.  sq(2,npoin_q) += (W, D);
// sv(npoin,L) += eps; part, if not NULL: the element partials [3L+2][ne]; row, if not NULL: the 3L+2
// integrals.  part and row need each other's loop only: either may be NULL.
template <int NGL>
inline void energy_host_ngl(const EnergyHost &g, double *sq, double *sv, double *part, double *row) {
  constexpr int NQ = 2 * NGL - 1, P = NGL * NGL, Q = NQ * NQ;
  const int L = g.L, R = en_rows(L);
  const bool series = part || row;
  std::vector<double> own;
  if (series && !part) {
    own.assign((size_t)R * g.ne, 0.0);
    part = own.data();
  }
  double ag[EN_MAXL], c[EN_MAXL];
  for (int k = 0; k < L; k++) {
    ag[k] = g.alpha[k] / g.gravity;
    c[k] = en_c(g.alpha, k, g.gravity);
  }
  std::vector<double> tile((size_t)(2 * L + 1) * P), mm((size_t)L * P), t((size_t)5 * NQ * NGL), prod((size_t)R * Q);
  for (int e = 0; e < g.ne; e++) {
    double *su = tile.data(), *sv_t = su + (size_t)L * P, *sdp = sv_t + (size_t)L * P;
    // phase 1: the nodes
    for (int ln = 0; ln < P; ln++) {
      const size_t I = (size_t)e * P + ln;
      double h[EN_MAXL], z[EN_MAXL];
      for (int k = 0; k < L; k++) {
        double dp, u, v, m;
        en_node(g.q + 3 * (I + g.npoin * k), g.gravity, dp, u, v, m);
        h[k] = ag[k] * dp;
        su[k * P + ln] = u;
        sv_t[k * P + ln] = v;
        mm[k * P + ln] = m;
        if (k == L - 1) sdp[ln] = dp;
        if (series) prod[(size_t)k * Q + ln] = g.w[I] * en_ke(u, v, m);
      }
      if (series) {
        double elev = g.zbot[I];
        for (int k = L - 1; k >= 0; k--) {
          elev = elev + h[k];
          z[k] = elev;
        }
        for (int k = 0; k < L; k++)
          prod[(size_t)(L + k) * Q + ln] = g.w[I] * en_ape(c[k], z[k], g.zref ? g.zref[I + g.npoin * k] : 0.0);
      }
    }
    // phase 2: the gradient and the dissipation
    for (int ln = 0; ln < P; ln++) {
      const size_t I = (size_t)e * P + ln;
      const int j = ln / NGL, i = ln - j * NGL;
      for (int k = 0; k < L; k++) {
        double u_x, u_y, v_x, v_y;
        en_grad<NGL>(su + k * P, sv_t + k * P, i, j, g.dpsi, g.ex[I], g.ey[I], g.nx[I], g.ny[I], u_x, u_y, v_x, v_y);
        const double eps = en_eps(g.visc, u_x, u_y, v_x, v_y, mm[k * P + ln]);
        sv[I + g.npoin * k] = sv[I + g.npoin * k] + eps;
        if (series) prod[(size_t)(2 * L + k) * Q + ln] = g.w[I] * eps;
      }
    }
    // phase 3: the first pass, t(iq,n) at [f][n*NQ + iq]
    const double *fld[5] = {su, sv_t, su + (size_t)(L - 1) * P, sv_t + (size_t)(L - 1) * P, sdp};
    const int nf = g.botfr ? 5 : 2;
    for (int f = 0; f < nf; f++)
      for (int n = 0; n < NGL; n++)
        for (int iq = 0; iq < NQ; iq++) {
          double ps[NGL];
          for (int m = 0; m < NGL; m++) ps[m] = g.psiq[m * NQ + iq];
          t[((size_t)f * NGL + n) * NQ + iq] = en_dot<NGL>(ps, fld[f] + n * NGL, 1);
        }
    // phase 4: the second pass, the wind work and the drag
    for (int lq = 0; lq < Q; lq++) {
      const size_t Iq = (size_t)e * Q + lq;
      const int jq = lq / NQ, iq = lq - jq * NQ;
      double ps[NGL], A[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int n = 0; n < NGL; n++) ps[n] = g.psiq[n * NQ + jq];
      for (int f = 0; f < nf; f++) A[f] = en_dot<NGL>(ps, t.data() + (size_t)f * NGL * NQ + iq, NQ);
      const double W = en_wind(g.tau[2 * Iq], g.tau[2 * Iq + 1], A[0], A[1]);
      const double aL = g.alpha[L - 1];
      const double D = g.botfr == 1   ? en_drag<1>(g.cd, g.gravity, aL, A[2], A[3], A[4])
                       : g.botfr == 2 ? en_drag<2>(g.cd, g.gravity, aL, A[2], A[3], A[4])
                                      : 0.0;
      sq[2 * Iq] = sq[2 * Iq] + W;
      sq[2 * Iq + 1] = sq[2 * Iq + 1] + D;
      if (series) {
        prod[(size_t)(3 * L) * Q + lq] = g.wq[Iq] * W;
        prod[(size_t)(3 * L + 1) * Q + lq] = g.wq[Iq] * D;
      }
    }
    // phase 5: the element partials, in order from the first product
    if (series)
      for (int r = 0; r < R; r++) {
        const int n = r < 3 * L ? P : Q;
        double s = prod[(size_t)r * Q];
        for (int x = 1; x < n; x++) s = s + prod[(size_t)r * Q + x];
        part[(size_t)r * g.ne + e] = s;
      }
  }
  if (row)
    for (int r = 0; r < R; r++) row[r] = en_tree_sum(std::vector<double>(part + (size_t)r * g.ne, part + (size_t)(r + 1) * g.ne));
}

// false: no such ngl (3, 4, 5, 6 or 8) or nlayers (1..3)
inline bool energy_host(const EnergyHost &g, double *sq, double *sv, double *part, double *row) {
  if (g.L < 1 || g.L > EN_MAXL || g.botfr < 0 || g.botfr > 2) return false;
  switch (g.ngl) {
    case 3: energy_host_ngl<3>(g, sq, sv, part, row); return true;
    case 4: energy_host_ngl<4>(g, sq, sv, part, row); return true;
    case 5: energy_host_ngl<5>(g, sq, sv, part, row); return true;
    case 6: energy_host_ngl<6>(g, sq, sv, part, row); return true;
    case 8: energy_host_ngl<8>(g, sq, sv, part, row); return true;
    default: return false;
  }
}

}  // namespace hnumo
