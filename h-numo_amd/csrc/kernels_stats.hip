// kernels_stats.hip -- online flow statistics on the engine's device state.
//
// What the double-gyre post-processing (Examples/double_gyre/compute_eke.m, compute_ke.m) forms
// from hundreds of mlswe#### snapshots, accumulated where the state lives: per owned node I and
// layer k, from q_df(3,npoin,L) exactly as diag_layer_fields (kernels_diag.hip) forms them,
//
//   dp = q(1);  h = (alpha_k/gravity)*dp (quotient first);  u = q(2)/dp;  v = q(3)/dp
//   uh = u*h;   vh = v*h;   e = (0.5*(u*u + v*v))*h
//
// One SAMPLE adds h, uh, vh, e to the running sums S_h, S_uh, S_vh, S_e (plain adds in sample
// order from +0.0; one lane owns a node's sums, so the order in time is the only order).  The
// finalised fields (5,npoin,L) after n samples:
//
//   hbar = S_h/double(n);  um = S_uh/S_h;  vm = S_vh/S_h;  mke = S_e/S_h
//   eke  = mke - 0.5*(um*um + vm*vm)
//
// The series holds per sample and layer KE_k = integral of e and VOL_k = integral of h over the
// rank's owned elements in a fixed order: per element the products w_I*e_I (w: the nodal jac) added
// one after the other in node order from the first product; the element sums combined by a
// position-based pairwise tree over the elements 0..ne-1 (entry i of the next level is x[2i] +
// x[2i+1], or x[2i] alone where 2i+1 does not exist).  The tree is defined by position, so the
// aligned power-of-two chunks of stats_tree_kernel give the bits of the whole tree.  No
// floating-point atomics.  Built with -ffp-contract=off: no FMA; IEEE division.  The host mirror
// of all of it is hnumo/flowstats.py (HostFlowStats), equal bit for bit.
//
// Layout of the sums: [L][2][npoin] pairs of doubles, pair 0 = (S_h, S_uh), pair 1 = (S_vh, S_e):
// lane i of a wave reads and writes 16 bytes at base + 16*i, 1 KiB contiguous per instruction.
// Nodes of ghost elements are never visited: their sums stay +0.0 and their fields read 0.
#include "engine_internal.h"

namespace hnumo {

constexpr int ST_BS = 256;
constexpr int ST_CHUNK = 1024;   // elements (partials) per workgroup of stats_tree_kernel: a power of two

struct StatsArgs {
  const double *q;       // q_df(3,npoin,L)
  const double *alpha;   // alpha_mlswe(L)
  const double *w;       // nodal jac (npoin)
  double2 *sums;         // [L][2][npoin]
  double *part;          // element partials [2L][ne]: row 2k = w*e of layer k, row 2k+1 = w*h
  double gravity;
  int npoin, ne, ngl;    // ne: the owned elements
};

__host__ __device__ inline size_t st_pair(int k, int p, size_t I, size_t npoin) { return ((size_t)k * 2 + p) * npoin + I; }

// One sample.  A workgroup visits groups of EPB = 256/P whole elements, one lane per node (the
// lanes of a group are consecutive nodes): per layer three 8-byte loads of q at a 24-byte stride,
// which together use every byte of their lines, and two 16-byte loads and stores of the sums.
// SERIES: the lane also puts w*e and w*h into LDS and, after a barrier, one lane per (element,
// layer, quantity) adds the element's P products in node order and writes the element partial.
// Without SERIES there is no LDS and no barrier.
template <int L, bool SERIES>
__global__ void __launch_bounds__(ST_BS) stats_accumulate_kernel(StatsArgs a) {
  __shared__ double s_p[SERIES ? 2 * L : 1][SERIES ? ST_BS : 1];
  const int tid = threadIdx.x, P = a.ngl * a.ngl, EPB = ST_BS / P;
  const int ngroups = (a.ne + EPB - 1) / EPB;
  const size_t npoin = (size_t)a.npoin;
  double ag[L];
#pragma unroll
  for (int k = 0; k < L; k++) ag[k] = a.alpha[k] / a.gravity;

  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int e0 = grp * EPB;
    const int nel = min(EPB, a.ne - e0);          // the last group may be ragged
    if (tid < nel * P) {
      const size_t I = (size_t)e0 * P + tid;
      double w = 0.0;
      if (SERIES) w = a.w[I];
#pragma unroll
      for (int k = 0; k < L; k++) {
        const double *p = a.q + 3 * (I + npoin * k);
        const double dp = p[0];
        const double h = ag[k] * dp;
        const double u = p[1] / dp, v = p[2] / dp;
        const double uh = u * h, vh = v * h;
        const double e = (0.5 * (u * u + v * v)) * h;
        double2 *s0 = a.sums + st_pair(k, 0, I, npoin), *s1 = a.sums + st_pair(k, 1, I, npoin);
        double2 x = *s0, y = *s1;
        x.x = x.x + h;
        x.y = x.y + uh;
        y.x = y.x + vh;
        y.y = y.y + e;
        *s0 = x;
        *s1 = y;
        if (SERIES) {
          s_p[2 * k][tid] = w * e;
          s_p[2 * k + 1][tid] = w * h;
        }
      }
    }
    if (SERIES) {
      __syncthreads();
      // lane -> (element of the group, row): the element index runs fastest
      for (int t = tid; t < nel * 2 * L; t += ST_BS) {
        const int le = t % nel, r = t / nel;
        const double *s = s_p[r] + le * P;
        double sum = s[0];
        for (int n = 1; n < P; n++) sum = sum + s[n];
        a.part[(size_t)r * a.ne + e0 + le] = sum;
      }
      __syncthreads();
    }
  }
}

// The halving of one chunk: x[0..m) in LDS, m <= ST_CHUNK, filled by the workgroup's ST_BS lanes (the
// barrier after the fill is taken here); x[0] holds the chunk's value on return, visible to every lane.
// The one text of the tree: stats_tree_kernel and region_tree_kernel (kernels_region.hip) call it.
__device__ __forceinline__ void tree_halve(double *x, int m, int tid) {
  __syncthreads();
  while (m > 1) {
    const int h = (m + 1) >> 1;
    constexpr int PER = ST_CHUNK / 2 / ST_BS;
    double v[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) {
      const int i = tid + j * ST_BS;
      if (i < h) v[j] = 2 * i + 1 < m ? x[2 * i] + x[2 * i + 1] : x[2 * i];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; j++) {
      const int i = tid + j * ST_BS;
      if (i < h) x[i] = v[j];
    }
    __syncthreads();
    m = h;
  }
}

// The pairwise tree over positions.  Workgroup (c, r) reduces the aligned chunk c of ST_CHUNK
// entries of row r of `in` (n entries per row) to one value, out[r * orow + c]: that value is entry c
// of level log2(ST_CHUNK) of the whole tree, so a pass over the chunks followed by passes over the
// results (the last one a single workgroup per row, writing the sample's slot of the series:
// orow = 1) is the tree of the definition.
__global__ void __launch_bounds__(ST_BS) stats_tree_kernel(const double *__restrict__ in, int n, double *__restrict__ out,
                                                           int orow) {
  __shared__ double x[ST_CHUNK];
  const int tid = threadIdx.x, c = blockIdx.x, r = blockIdx.y;
  const int base = c * ST_CHUNK;
  const int m = min(ST_CHUNK, n - base);
  const double *p = in + (size_t)r * n + base;
  for (int i = tid; i < m; i += ST_BS) x[i] = p[i];
  tree_halve(x, m, tid);
  if (tid == 0) out[(size_t)r * orow + c] = x[0];
}

// The finalised fields out(5,npoin,L) = hbar, um, vm, mke, eke after n samples; 0 at the nodes of
// ghost elements (I >= nown).
template <int L>
__global__ void __launch_bounds__(ST_BS) stats_fields_kernel(const double2 *__restrict__ sums, size_t npoin, size_t nown,
                                                             double n, double *__restrict__ out5) {
  const size_t s = (size_t)gridDim.x * blockDim.x;
  for (size_t I = (size_t)blockIdx.x * blockDim.x + threadIdx.x; I < npoin; I += s) {
#pragma unroll
    for (int k = 0; k < L; k++) {
      double f[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      if (I < nown) {
        const double2 x = sums[st_pair(k, 0, I, npoin)], y = sums[st_pair(k, 1, I, npoin)];
        const double um = x.y / x.x, vm = y.x / x.x, mke = y.y / x.x;
        f[0] = x.x / n;
        f[1] = um;
        f[2] = vm;
        f[3] = mke;
        f[4] = mke - 0.5 * (um * um + vm * vm);
      }
#pragma unroll
      for (int c = 0; c < 5; c++) out5[5 * (I + npoin * k) + c] = f[c];
    }
  }
}

}  // namespace hnumo
