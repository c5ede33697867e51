// kernels_diag.hip -- the reference's run diagnostics on the engine's device state.
//
//   layer fields (h, u, v, dp, ssh)   diagnostics.F90:24-45             diag_layer_fields, diag_fields_kernel
//   max/min of the layer fields, qb   print_diagnostics.F90:60-86       diag_reduce_kernel + diag_final_kernel
//   CFL_B, CFL                        courant.F90:34-127                diag_reduce_kernel + diag_final_kernel
//   layer mass                        compute_conserved.F90:29-41       diag_mass_kernel
//
// What mod_time_loop.F90:219-254 reports every irestart steps, formed from q_df(3,npoin,L) and
// qb_df(4,npoin) where they live, so that a report costs a read of the state instead of its copy
// to the host (hnumo_sync) and a single-threaded pass there.  Every value has the bits of the
// host restatement (hnumo/diagnostics.py), which is pinned to the reference: the arithmetic is
// the cited lines' with their grouping (built with -ffp-contract=off: no FMA; IEEE division).
// Max and min are exact, so those reductions run in any order: per lane over the elements a
// workgroup visits, over the workgroup by shuffles, over the workgroups in diag_final_kernel (no
// floating-point atomics).  The layer mass is the one ordered sum, kept in the reference's node
// order by diag_mass_kernel.
//
// The Courant numbers divide by the reference's RUNNING minimum cell size -- the minimum over the
// cells up to and including the one at hand in its loop order (courant.F90:98-102), not the
// grid's minimum.  It depends on the coordinates alone: hnumo_diag_geometry forms it once per
// cell on the host (cdx, cdy) and the maximum over the cells is then order-free.
#include "engine_internal.h"

namespace hnumo {

// A workgroup's partial results, and the final pass's input [dg_nv(L)][workgroups]:
//   maxima  0 cfl_b, 1 cfl, 2..5 qb(1:4), 6 + 5k + c field c of layer k
//   minima  dg_nmax(L) + (0..3 qb(1:4), 4 + 5k + c field c of layer k)
__host__ __device__ constexpr int dg_nmax(int L) { return 6 + 5 * L; }
__host__ __device__ constexpr int dg_nmin(int L) { return 4 + 5 * L; }
__host__ __device__ constexpr int dg_nv(int L) { return dg_nmax(L) + dg_nmin(L); }
// hnumo_diagnostics' out array: [cfl_b, cfl, min_dx, min_dy, qbmax(4), qbmin(4)], then per layer
// [mass, qmax(5), qmin(5)]
__host__ __device__ constexpr int dg_nout(int L) { return 12 + 11 * L; }
__host__ __device__ constexpr int dg_out_mass(int k) { return 12 + 11 * k; }

constexpr int DG_BS = 256;
constexpr double DG_CFL0 = -1.0e10;   // courant.F90:64-65

struct DiagArgs {
  const double *q, *qb;     // q_df(3,npoin,L), qb_df(4,npoin)
  const double *zbot;       // zbot_df(npoin)
  const double *alpha;      // alpha_mlswe(L)
  const double *cdx, *cdy;  // running minima of the cell sizes [ne][ngl-1][ngl-1]
  double gravity, dt, dt_btp;
  int npoin, ne, ngl;       // ne: the elements that count (the owned ones of a ghost-layer partition)
};

// f[k][0..4] = h, u, v, dp and the elevation of the layer's top interface at node I
// (diagnostics.F90:24-45): h = (alpha_k/g)*dp with the quotient first, the elevations summed
// upward from zbot_df
template <int L>
__device__ __forceinline__ void diag_layer_fields(const double *__restrict__ q, const double (&ag)[L], double zb,
                                                  size_t I, size_t npoin, double (&f)[L][5]) {
#pragma unroll
  for (int k = 0; k < L; k++) {
    const double *p = q + 3 * (I + npoin * k);
    const double dp = p[0];
    f[k][0] = ag[k] * dp;
    f[k][1] = p[1] / dp;
    f[k][2] = p[2] / dp;
    f[k][3] = dp;
  }
  double elev = zb;
#pragma unroll
  for (int k = L - 1; k >= 0; k--) {
    elev = elev + f[k][0];
    f[k][4] = elev;
  }
}

__device__ __forceinline__ double diag_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double diag_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}

// q(5,npoin,L) of diagnostics.F90:24-45, whole (hnumo_layer_fields)
template <int L>
__global__ void __launch_bounds__(DG_BS) diag_fields_kernel(DiagArgs a, double *__restrict__ out5) {
  double ag[L];
#pragma unroll
  for (int k = 0; k < L; k++) ag[k] = a.alpha[k] / a.gravity;
  const size_t npoin = (size_t)a.npoin, s = (size_t)gridDim.x * blockDim.x;
  for (size_t I = (size_t)blockIdx.x * blockDim.x + threadIdx.x; I < npoin; I += s) {
    double f[L][5];
    diag_layer_fields<L>(a.q, ag, a.zbot[I], I, npoin, f);
#pragma unroll
    for (int k = 0; k < L; k++)
#pragma unroll
      for (int c = 0; c < 5; c++) out5[5 * (I + npoin * k) + c] = f[k][c];
  }
}

// Extrema and Courant numbers.  A workgroup visits groups of EPB = 256/P whole elements, one lane
// per node: the lane forms its node's layer fields in registers and folds them and qb into its
// running maxima and minima; u_k, v_k and qb(3:4) go to LDS, and the lanes of the nodes (i, j) with
// i, j < ngl-1 then form the sub-cell's corner averages in the reference's order m = 1..4 =
// (i,j), (i+1,j), (i,j+1), (i+1,j+1), each term divided by 4 before it is added (courant.F90:77-93,
// 109-117).  One read of q, qb, zbot and the cell minima.
template <int L>
__global__ void __launch_bounds__(DG_BS) diag_reduce_kernel(DiagArgs a, double *__restrict__ part) {
  constexpr int NMAX = dg_nmax(L), NMIN = dg_nmin(L), NV = dg_nv(L);
  __shared__ double s_uv[2 * L + 2][DG_BS];
  __shared__ double s_red[DG_BS / 64][NV];
  const int tid = threadIdx.x, ngl = a.ngl, P = ngl * ngl, nc = ngl - 1, EPB = DG_BS / P;
  const int le = tid / P, ln = tid % P, j = ln / ngl, i = ln % ngl;
  const int ngroups = (a.ne + EPB - 1) / EPB;
  const size_t npoin = (size_t)a.npoin;
  double ag[L];
#pragma unroll
  for (int k = 0; k < L; k++) ag[k] = a.alpha[k] / a.gravity;
  double vmax[NMAX], vmin[NMIN];
  vmax[0] = vmax[1] = DG_CFL0;
#pragma unroll
  for (int v = 2; v < NMAX; v++) vmax[v] = -INFINITY;
#pragma unroll
  for (int v = 0; v < NMIN; v++) vmin[v] = INFINITY;

  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int e = grp * EPB + le;
    const bool act = le < EPB && e < a.ne;
    if (act) {
      const size_t I = (size_t)e * P + ln;
      double f[L][5];
      diag_layer_fields<L>(a.q, ag, a.zbot[I], I, npoin, f);
      const double *b = a.qb + 4 * I;
      const double b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
      vmax[2] = fmax(vmax[2], b0), vmin[0] = fmin(vmin[0], b0);
      vmax[3] = fmax(vmax[3], b1), vmin[1] = fmin(vmin[1], b1);
      vmax[4] = fmax(vmax[4], b2), vmin[2] = fmin(vmin[2], b2);
      vmax[5] = fmax(vmax[5], b3), vmin[3] = fmin(vmin[3], b3);
#pragma unroll
      for (int k = 0; k < L; k++) {
#pragma unroll
        for (int c = 0; c < 5; c++) {
          vmax[6 + 5 * k + c] = fmax(vmax[6 + 5 * k + c], f[k][c]);
          vmin[4 + 5 * k + c] = fmin(vmin[4 + 5 * k + c], f[k][c]);
        }
        s_uv[2 * k][tid] = f[k][1];
        s_uv[2 * k + 1][tid] = f[k][2];
      }
      s_uv[2 * L][tid] = b2;
      s_uv[2 * L + 1][tid] = b3;
    }
    __syncthreads();
    if (act && i < nc && j < nc) {
      // the corners' lanes: same element, so tid + 1 + ngl <= the element's last lane
      const int t2 = tid + 1, t3 = tid + ngl, t4 = tid + ngl + 1;
      const size_t c = ((size_t)e * nc + j) * nc + i;
      const double mdx = a.cdx[c], mdy = a.cdy[c];
      auto avg = [&](const double *s) {
        double r = 0.0;
        r = r + s[tid] / 4.0;
        r = r + s[t2] / 4.0;
        r = r + s[t3] / 4.0;
        r = r + s[t4] / 4.0;
        return r;
      };
      const double ub = avg(s_uv[2 * L]), vb = avg(s_uv[2 * L + 1]);
      vmax[0] = fmax(vmax[0], fabs(ub) * a.dt_btp / mdx);   // courant.F90:101-102
      vmax[0] = fmax(vmax[0], fabs(vb) * a.dt_btp / mdy);
#pragma unroll
      for (int k = 0; k < L; k++) {
        const double uk = avg(s_uv[2 * k]), vk = avg(s_uv[2 * k + 1]);
        vmax[1] = fmax(fabs(uk) * a.dt / mdx, vmax[1]);     // :119-120
        vmax[1] = fmax(fabs(vk) * a.dt / mdy, vmax[1]);
      }
    }
    __syncthreads();
  }

  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int v = 0; v < NMAX; v++) {
    const double r = diag_wave_max(vmax[v]);
    if (lane == 0) s_red[wave][v] = r;
  }
#pragma unroll
  for (int v = 0; v < NMIN; v++) {
    const double r = diag_wave_min(vmin[v]);
    if (lane == 0) s_red[wave][NMAX + v] = r;
  }
  __syncthreads();
  if (tid < NV) {
    double r = s_red[0][tid];
    for (int w = 1; w < DG_BS / 64; w++) r = tid < NMAX ? fmax(r, s_red[w][tid]) : fmin(r, s_red[w][tid]);
    part[(size_t)tid * gridDim.x + blockIdx.x] = r;
  }
}

// The pass over the workgroups' partial results: one wave per value, written to its place in
// hnumo_diagnostics' out array.
__global__ void __launch_bounds__(64) diag_final_kernel(const double *__restrict__ part, int nb, int L,
                                                        double *__restrict__ out) {
  const int v = blockIdx.x, lane = threadIdx.x, NMAX = dg_nmax(L);
  const bool is_max = v < NMAX;
  const double *p = part + (size_t)v * nb;
  double r = is_max ? (v < 2 ? DG_CFL0 : -INFINITY) : INFINITY;
  for (int b = lane; b < nb; b += 64) r = is_max ? fmax(r, p[b]) : fmin(r, p[b]);
  r = is_max ? diag_wave_max(r) : diag_wave_min(r);
  if (lane != 0) return;
  int o;
  if (v < 2)
    o = v;
  else if (v < 6)
    o = 4 + (v - 2);
  else if (is_max)
    o = dg_out_mass((v - 6) / 5) + 1 + (v - 6) % 5;
  else if (v - NMAX < 4)
    o = 8 + (v - NMAX);
  else
    o = dg_out_mass((v - NMAX - 4) / 5) + 6 + (v - NMAX - 4) % 5;
  out[o] = r;
}

// Layer mass (compute_conserved.F90:29-41): psih_df is the identity at the nodes, so layer k's
// mass is sum_I wjac_df(I) * h_k(I) added one node after the other in node order -- the order is
// the result (the reported mass loss is a difference near 1e-14 relative).  One workgroup per
// layer: all lanes form a chunk of products w*h (one multiply per node, as the reference) into
// LDS, lane 0 adds the chunk in order while the next chunk's loads are in flight.
constexpr int DG_MASS_PER = 8, DG_MASS_CH = DG_BS * DG_MASS_PER;
__global__ void __launch_bounds__(DG_BS) diag_mass_kernel(const double *__restrict__ q, const double *__restrict__ w,
                                                          const double *__restrict__ alpha, double gravity,
                                                          size_t npoin, size_t n, double *__restrict__ out) {
  __shared__ double buf[2][DG_MASS_CH];
  const int k = blockIdx.x, tid = threadIdx.x;
  const double ag = alpha[k] / gravity;
  const double *dp = q + 3 * npoin * k;
  const size_t nch = (n + DG_MASS_CH - 1) / DG_MASS_CH;
  double rw[DG_MASS_PER], rd[DG_MASS_PER];
  auto load = [&](size_t c) {
#pragma unroll
    for (int p = 0; p < DG_MASS_PER; p++) {
      const size_t I = c * DG_MASS_CH + (size_t)p * DG_BS + tid;
      rw[p] = I < n ? w[I] : 0.0;
      rd[p] = I < n ? dp[3 * I] : 0.0;
    }
  };
  auto stage = [&](double *b) {
#pragma unroll
    for (int p = 0; p < DG_MASS_PER; p++) b[p * DG_BS + tid] = rw[p] * (ag * rd[p]);
  };
  double sum = 0.0;
  if (nch > 0) {
    load(0);
    stage(buf[0]);
  }
  __syncthreads();
  for (size_t c = 0; c < nch; c++) {
    const bool more = c + 1 < nch;
    if (more) load(c + 1);
    if (tid == 0) {
      const double *b = buf[c & 1];
      const size_t left = n - c * DG_MASS_CH;
      const int cnt = left < (size_t)DG_MASS_CH ? (int)left : DG_MASS_CH;
      for (int t = 0; t < cnt; t++) sum = sum + b[t];
    }
    // (lane 0 is done with buf[c & 1] before its wave reaches the barrier, and no lane writes that
    // buffer again before passing it)
    if (more) stage(buf[(c + 1) & 1]);
    __syncthreads();
  }
  if (tid == 0) out[dg_out_mass(k)] = sum;
}

}  // namespace hnumo
