// kernels_vort.hip -- relative vorticity, divergence, layer potential vorticity and the Okubo-Weiss
// parameter of the engine's device state, with the enstrophy, potential-enstrophy and circulation
// series.
//
// The first products that take a derivative of the solution.  The reference stops short of them
// (write_output.F90:32,41 allocates `vorticity` and never fills it), so the arithmetic is defined
// here (normative; include/hnumo_engine.h).  Owned element e, layer k, node (i, j),
// I = e*P + j*ngl + i:
//
//   dp = q(1,I,k);  h = (alpha_k/gravity)*dp (quotient first);  u = q(2,I,k)/dp;  v = q(3,I,k)/dp
//   D(m,i) = dpsi(m,i) = l_m'(xgl_i)
//   u_xi = sum_m D(m,i)*u(m,j);  u_eta = sum_m D(m,j)*u(i,m)          (v likewise)
//   u_x = u_xi*ksi_x + u_eta*eta_x;  u_y = u_xi*ksi_y + u_eta*eta_y   (v likewise)
//   zeta = v_x - u_y;  delta = u_x + v_y;  pv = (zeta + f)/h
//   sn = u_x - v_y;  ss = v_x + u_y;  ow = (sn*sn + ss*ss) - zeta*zeta
//
// every sum left to right from its first product.  This is the element's own (broken) gradient: no
// face terms, so no halo and nothing between ranks; jumps at element edges are not lifted.  Series,
// per sample and layer: Z_k = integral of (0.5*(zeta*zeta))*h, PZ_k = integral of (0.5*(pv*pv))*h,
// G_k = integral of zeta over the rank's owned elements, summed as the flow statistics' series is
// (kernels_stats.hip): per element the products w_I*x_I in node order from the first one, the element
// sums by the position-defined pairwise tree (stats_tree_kernel).  No floating-point atomics.  Built
// with -ffp-contract=off: no FMA; IEEE division.  The host mirror is hnumo/vorticity.py
// (HostVorticity), equal bit for bit.  Nodes of ghost elements are never formed and read 0.
#include "engine_internal.h"

namespace hnumo {

constexpr int VT_BS = 256;

struct VortArgs {
  const double *q;       // q_df(3,npoin,L)
  const double *alpha;   // alpha_mlswe(L)
  const double *nstat;   // nodal statics [NS_N][npoin]: rows NS_EX..NS_NY (the metric terms), NS_W (jac)
  const double *f;       // coriolis_df(npoin), or NULL: 0
  const double *dpsi;    // D(m,i) at [m*ngl + i]
  double *out;           // fields, planar [L][4][npoin]: zeta, delta, pv, ow
  double *part;          // element partials [3L][ne]: rows 3k.. = Z, PZ, G of layer k (SERIES)
  double gravity;
  int npoin, ne;         // ne: the owned elements
};

// The element's own gradient at node (i, j).  su, sv: the element's u, v tiles in LDS (node (i, j) at
// [j*NGL + i]); Di[m] = D(m,i), Dj[m] = D(m,j); ex..ny = ksi_x, ksi_y, eta_x, eta_y.  The one text of the
// gradient: vort_node below and energy_sample_kernel (kernels_energy.hip) call it.
template <int NGL>
__device__ __forceinline__ void vort_grad(const double *su, const double *sv, int i, int j, const double (&Di)[NGL],
                                          const double (&Dj)[NGL], double ex, double ey, double nx, double ny, double &u_x,
                                          double &u_y, double &v_x, double &v_y) {
  const double *ur = su + j * NGL, *vr = sv + j * NGL, *uc = su + i, *vc = sv + i;
  double u_xi = Di[0] * ur[0], u_eta = Dj[0] * uc[0], v_xi = Di[0] * vr[0], v_eta = Dj[0] * vc[0];
#pragma unroll
  for (int m = 1; m < NGL; m++) {
    u_xi = u_xi + Di[m] * ur[m];
    u_eta = u_eta + Dj[m] * uc[m * NGL];
    v_xi = v_xi + Di[m] * vr[m];
    v_eta = v_eta + Dj[m] * vc[m * NGL];
  }
  u_x = u_xi * ex + u_eta * nx, u_y = u_xi * ey + u_eta * ny;
  v_x = v_xi * ex + v_eta * nx, v_y = v_xi * ey + v_eta * ny;
}

// The statements above for node (i, j) of one element (arguments as vort_grad's).  o = zeta, delta, pv, ow.
// The one text of the arithmetic: vort_kernel and sample_kernel's VORT source both call it.
template <int NGL>
__device__ __forceinline__ void vort_node(const double *su, const double *sv, int i, int j, const double (&Di)[NGL],
                                          const double (&Dj)[NGL], double ex, double ey, double nx, double ny, double f,
                                          double h, double (&o)[4]) {
  double u_x, u_y, v_x, v_y;
  vort_grad<NGL>(su, sv, i, j, Di, Dj, ex, ey, nx, ny, u_x, u_y, v_x, v_y);
  const double zeta = v_x - u_y;
  const double sn = u_x - v_y, ss = v_x + u_y;
  o[0] = zeta;
  o[1] = u_x + v_y;
  o[2] = (zeta + f) / h;
  o[3] = (sn * sn + ss * ss) - zeta * zeta;
}

// One pass over the owned elements.  A workgroup visits groups of EPB = 256/P whole elements, one
// lane per node, as stats_accumulate_kernel does.  Per group the lane loads its 24 bytes of q per
// layer, forms u, v, h and stores u, v of every layer into the LDS tiles; after one barrier it forms
// the four derivative sums per layer (a row and a column read of the tile; its 2 NGL entries of D sit
// in registers, loaded once per workgroup) and the six statements with the four metric rows and f,
// and writes the fields planar [L][4][npoin] (consecutive lanes, consecutive doubles).  A second
// barrier before the next group reuses the tiles.  The tiles are unpadded (a node's u at [tid], row
// stride NGL): a ds_read_b64 is banked per 32-lane half with bank (addr/4) mod 64, and the 32 lanes of
// a half hold 32 consecutive doubles of the tile -- the row read takes one address per row (broadcast
// along it; 4 rows, 16 banks apart, at NGL = 8), the column read NGL consecutive doubles per element
// (8 consecutive doubles at NGL = 8).  Enumerated over every half and m: no bank is met twice at
// NGL = 3, 4, 5, 8; at NGL = 6 the column read of a half that straddles two elements is 2-way (the
// elements lie 36 doubles apart).  No padding.
// SERIES: the lane also puts its three products per layer into LDS and, after the same barrier, one
// lane per (element, layer, quantity) adds the element's P products in node order and writes the
// element partial.  Without SERIES there are no partials and no LDS for them.
template <int NGL, int L, bool SERIES>
__global__ void __launch_bounds__(VT_BS) vort_kernel(VortArgs a) {
  constexpr int P = NGL * NGL, EPB = VT_BS / P;
  __shared__ double s_u[L][VT_BS], s_v[L][VT_BS];
  __shared__ double s_p[SERIES ? 3 * L : 1][SERIES ? VT_BS : 1];
  const int tid = threadIdx.x;
  const int le = tid / P, ln = tid - le * P, j = ln / NGL, i = ln - j * NGL;
  const int ngroups = (a.ne + EPB - 1) / EPB;
  const size_t npoin = (size_t)a.npoin;
  double ag[L], Di[NGL], Dj[NGL];
#pragma unroll
  for (int k = 0; k < L; k++) ag[k] = a.alpha[k] / a.gravity;
#pragma unroll
  for (int m = 0; m < NGL; m++) {
    Di[m] = a.dpsi[m * NGL + i];
    Dj[m] = a.dpsi[m * NGL + j];
  }

  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int e0 = grp * EPB;
    const int nel = min(EPB, a.ne - e0);          // the last group may be ragged
    const bool act = tid < nel * P;
    const size_t I = (size_t)e0 * P + tid;
    double h[L];
    if (act) {
#pragma unroll
      for (int k = 0; k < L; k++) {
        const double *p = a.q + 3 * (I + npoin * k);
        const double dp = p[0];
        h[k] = ag[k] * dp;
        s_u[k][tid] = p[1] / dp;
        s_v[k][tid] = p[2] / dp;
      }
    }
    __syncthreads();
    if (act) {
      const double ex = a.nstat[(size_t)NS_EX * npoin + I], ey = a.nstat[(size_t)NS_EY * npoin + I];
      const double nx = a.nstat[(size_t)NS_NX * npoin + I], ny = a.nstat[(size_t)NS_NY * npoin + I];
      const double f = a.f ? a.f[I] : 0.0;
      double w = 0.0;
      if (SERIES) w = a.nstat[(size_t)NS_W * npoin + I];
#pragma unroll
      for (int k = 0; k < L; k++) {
        double o[4];
        vort_node<NGL>(s_u[k] + le * P, s_v[k] + le * P, i, j, Di, Dj, ex, ey, nx, ny, f, h[k], o);
#pragma unroll
        for (int c = 0; c < 4; c++) a.out[((size_t)k * 4 + c) * npoin + I] = o[c];
        if (SERIES) {
          s_p[3 * k][tid] = w * ((0.5 * (o[0] * o[0])) * h[k]);
          s_p[3 * k + 1][tid] = w * ((0.5 * (o[2] * o[2])) * h[k]);
          s_p[3 * k + 2][tid] = w * o[0];
        }
      }
    }
    __syncthreads();
    if (SERIES) {
      // lane -> (element of the group, row): the element index runs fastest
      for (int t = tid; t < nel * 3 * L; t += VT_BS) {
        const int el = t % nel, r = t / nel;
        const double *s = s_p[r] + el * P;
        double sum = s[0];
        for (int n = 1; n < P; n++) sum = sum + s[n];
        a.part[(size_t)r * a.ne + e0 + el] = sum;
      }
      __syncthreads();
    }
  }
}

}  // namespace hnumo
