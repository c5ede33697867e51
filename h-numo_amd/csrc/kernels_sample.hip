// kernels_sample.hip -- the resident state, or the accumulated flow statistics, sampled at
// arbitrary points: the element's own Lagrange interpolant instead of a sync, a host pass over the
// nodes and a scattered-data interpolation (Examples/double_gyre/compute_ssh.m:58-70 and the other
// griddata scripts).
//
// A sample set is M points (element, xi, eta) with their 1-D weights Lx[i] = l_i(xi), Ly[j] =
// l_j(eta), formed once on the host (sample_plan.h).  Nodal fields F(e, j*ngl + i), node
// I = e*P + j*ngl + i:
//   source STATE  V = 5L + 4: rows 5k..5k+4 = h, u, v, dp, elevation of layer k as diag_layer_fields
//                 (kernels_diag.hip) forms them, rows 5L..5L+3 = qb_df(1:4, I)
//   source STATS  V = 5L: hbar, um, vm, mke, eke of layer k as stats_fields_kernel (kernels_stats.hip)
//                 forms them from the sums and the sample count
//   source VORT   V = 4L: zeta, delta, pv, ow of layer k as vort_node (kernels_vort.hip) forms them from
//                 the element's own u, v: passes of 256/P whole elements, one lane per node -- the lane
//                 stores u, v of every layer into the arena (rows 4k+2, 4k+3 of its element, which pv
//                 and ow overwrite afterwards), barrier, the shared function (zeta, delta to their rows
//                 at once, pv, ow into registers), barrier, the two rows.  The passes have the same trip count on every lane, so the barriers
//                 are reached by all; a station set costs its own few elements, not a pass over the
//                 field
//   source COV    V = 16L: the 16 fields of layer k as cov_node_fields (kernels_cov.hip) forms them from
//                 the covariances' sums and sample count (SampleArgs::sums, nsamp hold those then)
// Value: val = sum_j Ly[j] * r_j, r_j = sum_i Lx[i] * F(e, j*ngl + i), both sums left to right from
// their first product.  Points without an element read 0.0.  Built with -ffp-contract=off: no FMA;
// the host mirror is hnumo/sample.py (HostSampler), equal bit for bit.
//
// One 256-lane workgroup per chunk of the plan (at most 256 points in at most K distinct
// elements).  Phase 1: one lane per node of the chunk's elements forms the node's V fields into
// LDS -- the reads of q (three 8-byte loads at a 24-byte stride per layer), qb, zbot and the sums
// (two 16-byte loads per layer) have the shapes of diag_reduce_kernel and stats_accumulate_kernel,
// and every element is read once per chunk.  One barrier.  Phase 2: one lane per point reads its
// 2 ngl weights from the planar table (consecutive lanes, consecutive doubles), its element slot,
// evaluates the V double sums from LDS (lanes in one element read the same words: broadcasts) and
// writes out[v][perm]: planar [V][M], at the point's input position.  A chunk with at most 128
// points gives each point 2, 4 or 8 lanes, which share the V rows between them (a value is always
// one lane's sum: the bits do not depend on it).  No atomics, nothing between workgroups; every
// loop over registers has compile-time bounds.
#include "engine_internal.h"
#include "sample_plan.h"

namespace hnumo {

struct SampleArgs {
  const double *q, *qb, *zbot, *alpha;     // q_df(3,npoin,L), qb_df(4,npoin), zbot_df(npoin), alpha_mlswe(L)
  const double2 *sums;                     // the statistics' sums [L][2][npoin] (source STATS)
  double gravity, nsamp;                   // nsamp: the statistics' sample count
  const double *nstat, *f, *dpsi;          // source VORT: VortArgs' nstat, f (or NULL) and dpsi
  const int *chunk_pt, *chunk_el, *el_list, *slot, *perm;
  const double *w;                         // [2 ngl][M]
  double *out;                             // [V][M]
  size_t npoin, M;
};

// (the VORT source holds D, h and pv, ow across its barriers: four workgroups per CU leave it the
// registers for that without scratch at NGL = 8, L = 3; three leave the COV source those for its seven
// pairs and 16 fields per layer without scratch at NGL = 6; the other sources keep five)
template <int NGL, int L, int SRC>
__global__ void __launch_bounds__(SP_CHUNK, SRC == SP_SRC_COV ? 3 : SRC == SP_SRC_VORT ? 4 : 5) sample_kernel(SampleArgs a) {
  constexpr int P = NGL * NGL, V = sp_nval(L, SRC), ES = sp_estride(NGL, V), K = sp_K(NGL, V);
  static_assert(K >= 1, "the arena holds no element");
  __shared__ double s_f[K * ES];
  const int tid = threadIdx.x, c = blockIdx.x;
  const int el0 = a.chunk_el[c], nel = a.chunk_el[c + 1] - el0;
  const size_t npoin = a.npoin;

  double ag[L];
  if (SRC == SP_SRC_STATE || SRC == SP_SRC_VORT) {
#pragma unroll
    for (int k = 0; k < L; k++) ag[k] = a.alpha[k] / a.gravity;
  }
  if constexpr (SRC == SP_SRC_VORT) {
    constexpr int EPI = SP_CHUNK / P;              // whole elements per pass
    const int le0 = tid / P, ln = tid - le0 * P, j = ln / NGL, i = ln - j * NGL;
    for (int b = 0; b < nel; b += EPI) {           // (nel is the workgroup's: every lane makes every pass)
      const int le = b + le0;
      const bool act = tid < EPI * P && le < nel;
      double *s = s_f + (act ? le : 0) * ES + ln;
      size_t I = 0;
      double h[L], pvow[L][2];
      if (act) {
        I = (size_t)a.el_list[el0 + le] * P + ln;
#pragma unroll
        for (int k = 0; k < L; k++) {
          const double *p = a.q + 3 * (I + npoin * k);
          const double dp = p[0];
          h[k] = ag[k] * dp;
          s[(4 * k + 2) * P] = p[1] / dp;
          s[(4 * k + 3) * P] = p[2] / dp;
        }
      }
      __syncthreads();
      if (act) {
        // (D is read here, pass by pass, and zeta, delta go to their own rows at once: fewer
        // registers live across the barriers)
        double Di[NGL], Dj[NGL];
#pragma unroll
        for (int m = 0; m < NGL; m++) {
          Di[m] = a.dpsi[m * NGL + i];
          Dj[m] = a.dpsi[m * NGL + j];
        }
        const double ex = a.nstat[(size_t)NS_EX * npoin + I], ey = a.nstat[(size_t)NS_EY * npoin + I];
        const double nx = a.nstat[(size_t)NS_NX * npoin + I], ny = a.nstat[(size_t)NS_NY * npoin + I];
        const double f = a.f ? a.f[I] : 0.0;
        const double *se = s_f + le * ES;
#pragma unroll
        for (int k = 0; k < L; k++) {
          double o[4];
          vort_node<NGL>(se + (4 * k + 2) * P, se + (4 * k + 3) * P, i, j, Di, Dj, ex, ey, nx, ny, f, h[k], o);
          s[(4 * k) * P] = o[0];
          s[(4 * k + 1) * P] = o[1];
          pvow[k][0] = o[2];
          pvow[k][1] = o[3];
        }
      }
      __syncthreads();
      if (act) {
#pragma unroll
        for (int k = 0; k < L; k++) {
          s[(4 * k + 2) * P] = pvow[k][0];
          s[(4 * k + 3) * P] = pvow[k][1];
        }
      }
    }
  }
  for (int t = tid; SRC != SP_SRC_VORT && t < nel * P; t += SP_CHUNK) {
    const int le = t / P, ln = t - le * P;
    const size_t I = (size_t)a.el_list[el0 + le] * P + ln;
    double *s = s_f + le * ES + ln;
    if (SRC == SP_SRC_COV) {
#pragma unroll
      for (int k = 0; k < L; k++) {
        double f[CV_NFIELD];
        cov_node_fields(a.sums, k, I, npoin, a.nsamp, f);
#pragma unroll
        for (int v = 0; v < CV_NFIELD; v++) s[(CV_NFIELD * k + v) * P] = f[v];
      }
    } else if (SRC == SP_SRC_STATE) {
      double f[L][5];
      diag_layer_fields<L>(a.q, ag, a.zbot[I], I, npoin, f);
#pragma unroll
      for (int k = 0; k < L; k++)
#pragma unroll
        for (int v = 0; v < 5; v++) s[(5 * k + v) * P] = f[k][v];
      const double *b = a.qb + 4 * I;
#pragma unroll
      for (int v = 0; v < 4; v++) s[(5 * L + v) * P] = b[v];
    } else {
#pragma unroll
      for (int k = 0; k < L; k++) {
        const double2 x = a.sums[st_pair(k, 0, I, npoin)], y = a.sums[st_pair(k, 1, I, npoin)];
        const double um = x.y / x.x, vm = y.x / x.x, mke = y.y / x.x;
        s[(5 * k + 0) * P] = x.x / a.nsamp;
        s[(5 * k + 1) * P] = um;
        s[(5 * k + 2) * P] = vm;
        s[(5 * k + 3) * P] = mke;
        s[(5 * k + 4) * P] = mke - 0.5 * (um * um + vm * vm);
      }
    }
  }
  __syncthreads();

  // G lanes per point (a power of two, the same for the whole chunk): a chunk cut short by its K
  // elements has few points, and its V rows are then dealt out to the lanes that would idle --
  // lane g of a point evaluates rows g, g + G, ...; every value is still one lane's sum
  const int pt0 = a.chunk_pt[c], npts = a.chunk_pt[c + 1] - pt0;
  int lg = 0;
  while (lg < 3 && (npts << (lg + 1)) <= SP_CHUNK) lg++;
  const int G = 1 << lg, g = tid & (G - 1);
  if ((tid >> lg) >= npts) return;
  const size_t sp = (size_t)pt0 + (tid >> lg);
  const int sl = a.slot[sp];
  double *o = a.out + a.perm[sp];
  if (sl < 0) {
    for (int v = g; v < V; v += G) o[(size_t)v * a.M] = 0.0;
    return;
  }
  double lx[NGL], ly[NGL];
#pragma unroll
  for (int i = 0; i < NGL; i++) {
    lx[i] = a.w[(size_t)i * a.M + sp];
    ly[i] = a.w[(size_t)(NGL + i) * a.M + sp];
  }
  for (int v = g; v < V; v += G) {
    const double *f = s_f + sl * ES + v * P;
    double val = 0.0;
#pragma unroll
    for (int j = 0; j < NGL; j++) {
      double r = lx[0] * f[j * NGL];
#pragma unroll
      for (int i = 1; i < NGL; i++) r = r + lx[i] * f[j * NGL + i];
      val = j == 0 ? ly[0] * r : val + ly[j] * r;
    }
    o[(size_t)v * a.M] = val;
  }
}

}  // namespace hnumo
