// kernels_cov.hip -- eddy covariances of the engine's device state: the thickness-weighted Reynolds
// stresses, the eddy thickness flux, the interface (SSH) variance, the eddy potential-vorticity flux and
// the eddy potential enstrophy, accumulated where the state lives.
//
// Definitions (normative; include/hnumo_engine.h).  Per owned node I of element e and
// layer k, per sample:
//
//   dp, h, u, v   as hnumo_stats / hnumo_vort form them (h = (alpha_k/gravity)*dp, quotient first;
//                 u = q2/dp; v = q3/dp)
//   z             = elevation of layer k's top interface as hnumo_layer_fields forms it (row 5; summed
//                   upward from zbot_df)
//   d             = z - zref(I,k)                  (zref given at begin, NULL: 0.0)
//   zeta, pv      = o[0], o[2] of vort_node for this node and layer (f as given at begin, NULL: 0.0)
//   a             = zeta + f(I)
//
// One SAMPLE adds these 14 terms to running sums (plain adds in sample order from +0.0; one lane owns a
// node's sums, so the order in time is the only order):
//
//   S_h  += h        S_u  += u          S_v  += v
//   S_uh += u*h      S_vh += v*h
//   S_uuh += (u*u)*h S_uvh += (u*v)*h   S_vvh += (v*v)*h
//   S_d  += d        S_dd += d*d
//   S_a  += a        S_ua += u*a        S_va += v*a        S_qa += pv*a
//
// The fields, 16 per node and layer, after n samples with N = double(n):
//
//   hbar = S_h/N   ubar = S_u/N   vbar = S_v/N   um = S_uh/S_h   vm = S_vh/S_h
//   Ruu = S_uuh/S_h - um*um    Ruv = S_uvh/S_h - um*vm    Rvv = S_vvh/S_h - vm*vm
//   Fu  = S_uh/N - ubar*hbar   Fv  = S_vh/N - vbar*hbar
//   dbar = S_d/N               dvar = S_dd/N - dbar*dbar
//   qm  = S_a/S_h              Qu  = S_ua/S_h - um*qm     Qv = S_va/S_h - vm*qm
//   ens = 0.5*(S_qa/S_h - qm*qm)
//
// The integrals, per layer: of hbar*(0.5*(Ruu+Rvv)), of dvar and of hbar*ens over the rank's owned
// elements, summed as the flow statistics' series is (kernels_stats.hip): per element the products
// w_I*x_I (w: the nodal jac) in node order from the first one, the element sums by the position-defined
// pairwise tree (stats_tree_kernel).  No floating-point atomics.  Built with -ffp-contract=off: no FMA;
// IEEE division; every sum left to right.  The host mirror is hnumo/covariance.py (HostEddyCov), equal
// bit for bit.  Nodes of ghost elements are never accumulated: their sums stay +0.0 and their fields
// read 0.
//
// Layout of the sums: [L][7][npoin] pairs of doubles, pair p of a layer = sums 2p and 2p+1 in the order
// S_h, S_u, S_v, S_uh, S_vh, S_uuh, S_uvh, S_vvh, S_d, S_dd, S_a, S_ua, S_va, S_qa: lane i of a wave
// reads and writes 16 bytes at base + 16*i, the streams of stats_accumulate_kernel, seven per layer.
#include "engine_internal.h"

namespace hnumo {

constexpr int CV_BS = 256;
constexpr int CV_NSUM = 14, CV_NPAIR = 7, CV_NFIELD = 16, CV_NINT = 3;

struct CovArgs {
  const double *q;       // q_df(3,npoin,L)
  const double *alpha;   // alpha_mlswe(L)
  const double *nstat;   // nodal statics [NS_N][npoin]: the metric rows, NS_W (jac), NS_ZB (zbot_df)
  const double *f;       // coriolis_df(npoin), or NULL: 0
  const double *zref;    // zref(npoin,L), or NULL: 0
  const double *dpsi;    // D(m,i) at [m*ngl + i]
  double2 *sums;         // [L][7][npoin]
  double *part;          // element partials [3L][ne] (cov_integrals_kernel)
  double gravity, nsamp; // nsamp: double(n), the sample count (cov_integrals_kernel)
  int npoin, ne, ngl;    // ne: the owned elements
};

__host__ __device__ inline size_t cv_pair(int k, int p, size_t I, size_t npoin) { return ((size_t)k * CV_NPAIR + p) * npoin + I; }

// One sample.  A workgroup visits groups of EPB = 256/P whole elements, one lane per node, as
// vort_kernel does: the lane loads its 24 bytes of q per layer, forms h, u, v and stores u, v of every
// layer into the unpadded LDS tiles (the banking argument of vort_kernel carries over: the tiles, the
// row read and the column read are the same); after one barrier vort_node gives zeta and pv per layer
// (delta and ow are dead and dropped by the compiler), the lane adds the thicknesses upward from zbot
// for the elevations and then, layer by layer, reads, adds and writes its seven pairs.  A second barrier
// before the next group reuses the tiles.
template <int NGL, int L>
__global__ void __launch_bounds__(CV_BS) cov_accumulate_kernel(CovArgs a) {
  constexpr int P = NGL * NGL, EPB = CV_BS / P;
  __shared__ double s_u[L][CV_BS], s_v[L][CV_BS];
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
    double h[L], u[L], v[L];
    if (act) {
#pragma unroll
      for (int k = 0; k < L; k++) {
        const double *p = a.q + 3 * (I + npoin * k);
        const double dp = p[0];
        h[k] = ag[k] * dp;
        u[k] = p[1] / dp;
        v[k] = p[2] / dp;
        s_u[k][tid] = u[k];
        s_v[k][tid] = v[k];
      }
    }
    __syncthreads();
    if (act) {
      const double ex = a.nstat[(size_t)NS_EX * npoin + I], ey = a.nstat[(size_t)NS_EY * npoin + I];
      const double nx = a.nstat[(size_t)NS_NX * npoin + I], ny = a.nstat[(size_t)NS_NY * npoin + I];
      const double f = a.f ? a.f[I] : 0.0;
      double z[L];
      double elev = a.nstat[(size_t)NS_ZB * npoin + I];
#pragma unroll
      for (int k = L - 1; k >= 0; k--) {
        elev = elev + h[k];
        z[k] = elev;
      }
#pragma unroll
      for (int k = 0; k < L; k++) {
        double o[4];
        vort_node<NGL>(s_u[k] + le * P, s_v[k] + le * P, i, j, Di, Dj, ex, ey, nx, ny, f, h[k], o);
        const double av = o[0] + f, pv = o[2];
        const double d = z[k] - (a.zref ? a.zref[I + npoin * k] : 0.0);
        const double hk = h[k], uk = u[k], vk = v[k];
        double2 *s = a.sums + cv_pair(k, 0, I, npoin);
        double2 x0 = s[0], x1 = s[npoin], x2 = s[2 * npoin], x3 = s[3 * npoin];
        double2 x4 = s[4 * npoin], x5 = s[5 * npoin], x6 = s[6 * npoin];
        x0.x = x0.x + hk;
        x0.y = x0.y + uk;
        x1.x = x1.x + vk;
        x1.y = x1.y + uk * hk;
        x2.x = x2.x + vk * hk;
        x2.y = x2.y + (uk * uk) * hk;
        x3.x = x3.x + (uk * vk) * hk;
        x3.y = x3.y + (vk * vk) * hk;
        x4.x = x4.x + d;
        x4.y = x4.y + d * d;
        x5.x = x5.x + av;
        x5.y = x5.y + uk * av;
        x6.x = x6.x + vk * av;
        x6.y = x6.y + pv * av;
        s[0] = x0;
        s[npoin] = x1;
        s[2 * npoin] = x2;
        s[3 * npoin] = x3;
        s[4 * npoin] = x4;
        s[5 * npoin] = x5;
        s[6 * npoin] = x6;
      }
    }
    __syncthreads();
  }
}

// The 16 fields of node I, layer k from its seven pairs; n = double(samples).  The one text of the
// fields' arithmetic: cov_fields_kernel, cov_integrals_kernel and sample_kernel's COV source call it.
__device__ __forceinline__ void cov_node_fields(const double2 *__restrict__ sums, int k, size_t I, size_t npoin, double n,
                                                double (&o)[CV_NFIELD]) {
  const double2 *s = sums + cv_pair(k, 0, I, npoin);
  const double2 x0 = s[0], x1 = s[npoin], x2 = s[2 * npoin], x3 = s[3 * npoin];
  const double2 x4 = s[4 * npoin], x5 = s[5 * npoin], x6 = s[6 * npoin];
  const double Sh = x0.x, Su = x0.y, Sv = x1.x, Suh = x1.y, Svh = x2.x, Suuh = x2.y, Suvh = x3.x, Svvh = x3.y;
  const double Sd = x4.x, Sdd = x4.y, Sa = x5.x, Sua = x5.y, Sva = x6.x, Sqa = x6.y;
  const double hbar = Sh / n, ubar = Su / n, vbar = Sv / n, um = Suh / Sh, vm = Svh / Sh;
  const double dbar = Sd / n, qm = Sa / Sh;
  o[0] = hbar;
  o[1] = ubar;
  o[2] = vbar;
  o[3] = um;
  o[4] = vm;
  o[5] = Suuh / Sh - um * um;
  o[6] = Suvh / Sh - um * vm;
  o[7] = Svvh / Sh - vm * vm;
  o[8] = Suh / n - ubar * hbar;
  o[9] = Svh / n - vbar * hbar;
  o[10] = dbar;
  o[11] = Sdd / n - dbar * dbar;
  o[12] = qm;
  o[13] = Sua / Sh - um * qm;
  o[14] = Sva / Sh - vm * qm;
  o[15] = 0.5 * (Sqa / Sh - qm * qm);
}

// The fields out(16,npoin,L) after n samples; 0 at the nodes of ghost elements (I >= nown).
template <int L>
__global__ void __launch_bounds__(CV_BS) cov_fields_kernel(const double2 *__restrict__ sums, size_t npoin, size_t nown,
                                                           double n, double *__restrict__ out16) {
  const size_t s = (size_t)gridDim.x * blockDim.x;
  for (size_t I = (size_t)blockIdx.x * blockDim.x + threadIdx.x; I < npoin; I += s) {
#pragma unroll
    for (int k = 0; k < L; k++) {
      double f[CV_NFIELD];
#pragma unroll
      for (int c = 0; c < CV_NFIELD; c++) f[c] = 0.0;
      if (I < nown) cov_node_fields(sums, k, I, npoin, n, f);
#pragma unroll
      for (int c = 0; c < CV_NFIELD; c++) out16[CV_NFIELD * (I + npoin * k) + c] = f[c];
    }
  }
}

// The element partials [3L][ne] of the integrals: rows 3k.. = w*(hbar*(0.5*(Ruu+Rvv))), w*dvar,
// w*(hbar*ens) of layer k, per element added in node order from the first product -- the groups, the
// LDS rows and the adding lanes of stats_accumulate_kernel's series.
template <int L>
__global__ void __launch_bounds__(CV_BS) cov_integrals_kernel(CovArgs a) {
  __shared__ double s_p[CV_NINT * L][CV_BS];
  const int tid = threadIdx.x, P = a.ngl * a.ngl, EPB = CV_BS / P;
  const int ngroups = (a.ne + EPB - 1) / EPB;
  const size_t npoin = (size_t)a.npoin;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int e0 = grp * EPB;
    const int nel = min(EPB, a.ne - e0);          // the last group may be ragged
    if (tid < nel * P) {
      const size_t I = (size_t)e0 * P + tid;
      const double w = a.nstat[(size_t)NS_W * npoin + I];
#pragma unroll
      for (int k = 0; k < L; k++) {
        double f[CV_NFIELD];
        cov_node_fields(a.sums, k, I, npoin, a.nsamp, f);
        s_p[CV_NINT * k][tid] = w * (f[0] * (0.5 * (f[5] + f[7])));
        s_p[CV_NINT * k + 1][tid] = w * f[11];
        s_p[CV_NINT * k + 2][tid] = w * (f[0] * f[15]);
      }
    }
    __syncthreads();
    // lane -> (element of the group, row): the element index runs fastest
    for (int t = tid; t < nel * CV_NINT * L; t += CV_BS) {
      const int el = t % nel, r = t / nel;
      const double *s = s_p[r] + el * P;
      double sum = s[0];
      for (int n = 1; n < P; n++) sum = sum + s[n];
      a.part[(size_t)r * a.ne + e0 + el] = sum;
    }
    __syncthreads();
  }
}

}  // namespace hnumo
