// kernels_region.hip -- regional budgets of the engine's device state: per-region integral series by a
// segmented, position-defined tree reduction.
//
// Definitions (normative; include/hnumo_engine.h, DESIGN.md §6.1.9, region_plan.h, hnumo/regions.py).  A
// region set labels every owned element with a region r in 0..R; label 0: the element is in no region.
// Up to RG_MAXSETS sets exist at once (overlapping partitions, such as strips and basins, are separate
// sets).  The members of region r, in ascending local element number, have local positions 0..n_r-1.
// IEEE double, -ffp-contract=off: no FMA; IEEE division; every sum left to right from its first product.
// Per member element e, layer k, node I = e*P + j*ngl + i, w_I the nodal jac (NS_W):
//   FLOW rows (mask bit 0), the statements of §6.1.1:
//     dp = q(1); h = (alpha_k/gravity)*dp; u = q(2)/dp; v = q(3)/dp
//     VOL_k = int h;  TU_k = int (u*h);  TV_k = int (v*h);  KE_k = int ((0.5*(u*u+v*v))*h)
//   VORT rows (mask bit 1), the statements of §6.1.4 through vort_node (kernels_vort.hip), which stays the
//   one device text; f the caller's coriolis_df, 0 for NULL:
//     Z_k = int ((0.5*(zeta*zeta))*h);  PZ_k = int ((0.5*(pv*pv))*h);  G_k = int zeta
// `int` in two steps: per element the products w_I*x_I added in node order from the first product; per
// region the element sums combined by §6.1.1's pairwise tree over the LOCAL POSITIONS (entry i of the
// next level is x[2i] + x[2i+1], or x[2i] alone where 2i+1 does not exist).  An empty region reads +0.0
// in every row.  No floating-point atomics.  Ghost elements are never members.
// Entry: (V, R), V = 4L*[FLOW] + 3L*[VORT]; FLOW rows first, 4(k-1) + {0 VOL, 1 TU, 2 TV, 3 KE}, then the
// VORT rows, 3(k-1) + {0 Z, 1 PZ, 2 G} (hnumo_vort_series' order).  The host mirror is hnumo/regions.py
// (HostRegions), equal bit for bit.
//
// One sample is one region_accumulate_kernel over the member list and one region_tree_kernel per pass
// of the plan (region_plan.h): ceil(log_1024 max_r n_r) passes, at least one, whatever R is.
#include "engine_internal.h"

namespace hnumo {

constexpr int RG_BS = 256;
static_assert(RG_BS == ST_BS && RG_CHUNK == ST_CHUNK, "region_tree_kernel shares tree_halve with stats_tree_kernel");

struct RegionArgs {
  const double *q;       // q_df(3,npoin,L)
  const double *alpha;   // alpha_mlswe(L)
  const double *nstat;   // nodal statics [NS_N][npoin]: rows NS_EX..NS_NY (the metric terms), NS_W (jac)
  const double *f;       // coriolis_df(npoin), or NULL: 0
  const double *dpsi;    // D(m,i) at [m*ngl + i]
  const int *mem;        // the member list [nmem]: 0-based owned elements sorted by (region, element)
  double *part;          // element partials [V][nmem]: row v of member position s at [v*nmem + s]
  double gravity;
  int npoin, nmem;
};

// One pass over the MEMBER LIST: the cost follows the members, not the mesh, and a non-member is never
// loaded.  A workgroup visits groups of EPB = 256/P consecutive members, one lane per node (lane tid is
// node tid - le*P of the group's member le).  The lane loads its 24 bytes of q per layer (three 8-byte
// loads at a 24-byte stride, which together use every byte of their lines within an element; elements of
// a group are P*24 bytes long each and lie wherever the member list says) and forms h, u, v of every
// layer; with VORT it stores u, v of all layers into the LDS tiles and, after one barrier, calls vort_node.
// The products are staged LAYER BY LAYER: NR = 4*[FLOW] + 3*[VORT] rows of one layer go into LDS, one lane
// per (member, row) adds the member's P products in node order and writes the partial to
// [row][member position], and the rows are reused for the next layer.  All 7L rows at once would take
// 42 KiB at L = 3 beside the 12 KiB of tiles (2 workgroups per CU by LDS); one layer's rows take 14 KiB
// (6 per CU).  Consecutive members are consecutive positions, so each row's stores are contiguous.
// LDS banks.  The tiles are unpadded and read as vort_kernel reads them (a node's u at [tid], row stride
// NGL): a ds_read_b64 is banked per 32-lane half with bank (addr/4) mod 64, the 32 lanes of a half hold 32
// consecutive doubles of the tile, the row read takes one address per row (broadcast along it) and the
// column read NGL consecutive doubles per element -- no bank met twice at NGL = 3, 4, 5, 8, 2-way at
// NGL = 6 in a half that straddles two elements (§6.1.4).  The product rows give each member PS = P | 1
// doubles (P = 16, 36, 64 padded by one): the adding lanes of a half are consecutive members, PS doubles
// = 2*PS banks apart with PS odd, so 32 lanes meet 32 different even banks -- conflict-free, where the
// unpadded stride 16 (32 banks) would be 16-way.  The product stores are consecutive doubles with one
// skipped per member: conflict-free.
template <int NGL, int L, int ROWS>
__global__ void __launch_bounds__(RG_BS) region_accumulate_kernel(RegionArgs a) {
  constexpr int P = NGL * NGL, EPB = RG_BS / P, PS = P | 1;
  constexpr bool FLOW = (ROWS & RG_FLOW) != 0, VORT = (ROWS & RG_VORT) != 0;
  constexpr int NF = FLOW ? 4 : 0, NR = NF + (VORT ? 3 : 0), VB = rg_vort_base(L, ROWS);
  __shared__ double s_u[VORT ? L : 1][VORT ? RG_BS : 1], s_v[VORT ? L : 1][VORT ? RG_BS : 1];
  __shared__ double s_p[NR][EPB * PS];
  const int tid = threadIdx.x;
  const int le = tid / P, ln = tid - le * P, j = ln / NGL, i = ln - j * NGL;
  const int ngroups = (a.nmem + EPB - 1) / EPB;
  const size_t npoin = (size_t)a.npoin, nmem = (size_t)a.nmem;
  double ag[L], Di[NGL], Dj[NGL];
#pragma unroll
  for (int k = 0; k < L; k++) ag[k] = a.alpha[k] / a.gravity;
  if constexpr (VORT) {
#pragma unroll
    for (int m = 0; m < NGL; m++) {
      Di[m] = a.dpsi[m * NGL + i];
      Dj[m] = a.dpsi[m * NGL + j];
    }
  }

  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int s0 = grp * EPB;
    const int nel = min(EPB, a.nmem - s0);        // the last group may be ragged
    const bool act = tid < nel * P;
    size_t I = 0;
    double h[L], u[L], v[L];
    if (act) {
      I = (size_t)a.mem[s0 + le] * P + ln;
#pragma unroll
      for (int k = 0; k < L; k++) {
        const double *p = a.q + 3 * (I + npoin * k);
        const double dp = p[0];
        h[k] = ag[k] * dp;
        u[k] = p[1] / dp;
        v[k] = p[2] / dp;
        if constexpr (VORT) {
          s_u[k][tid] = u[k];
          s_v[k][tid] = v[k];
        }
      }
    }
    if constexpr (VORT) __syncthreads();
    double w = 0.0, ex = 0.0, ey = 0.0, nx = 0.0, ny = 0.0, f = 0.0;
    if (act) {
      w = a.nstat[(size_t)NS_W * npoin + I];
      if constexpr (VORT) {
        ex = a.nstat[(size_t)NS_EX * npoin + I], ey = a.nstat[(size_t)NS_EY * npoin + I];
        nx = a.nstat[(size_t)NS_NX * npoin + I], ny = a.nstat[(size_t)NS_NY * npoin + I];
        f = a.f ? a.f[I] : 0.0;
      }
    }
#pragma unroll
    for (int k = 0; k < L; k++) {
      if (act) {
        double *sp = &s_p[0][le * PS + ln];
        if constexpr (FLOW) {
          sp[0] = w * h[k];
          sp[EPB * PS] = w * (u[k] * h[k]);
          sp[2 * EPB * PS] = w * (v[k] * h[k]);
          sp[3 * EPB * PS] = w * ((0.5 * (u[k] * u[k] + v[k] * v[k])) * h[k]);
        }
        if constexpr (VORT) {
          double o[4];
          vort_node<NGL>(s_u[k] + le * P, s_v[k] + le * P, i, j, Di, Dj, ex, ey, nx, ny, f, h[k], o);
          sp[NF * EPB * PS] = w * ((0.5 * (o[0] * o[0])) * h[k]);
          sp[(NF + 1) * EPB * PS] = w * ((0.5 * (o[2] * o[2])) * h[k]);
          sp[(NF + 2) * EPB * PS] = w * o[0];
        }
      }
      __syncthreads();
      // lane -> (member of the group, row): the member index runs fastest
      for (int t = tid; t < nel * NR; t += RG_BS) {
        const int el = t % nel, r = t / nel;
        const double *s = s_p[r] + el * PS;
        double sum = s[0];
        for (int n = 1; n < P; n++) sum = sum + s[n];
        const int row = r < NF ? 4 * k + r : VB + 3 * k + (r - NF);
        a.part[(size_t)row * nmem + s0 + el] = sum;
      }
      __syncthreads();   // (the rows, and after the last layer the tiles, are written again)
    }
  }
}

// The members' areas: per member the products w_I*1.0 added in node order into part[0][member position];
// the same tree then gives sum w_I per region (hnumo_regions_area).  Once per set, at create.
__global__ void __launch_bounds__(RG_BS) region_area_kernel(const double *__restrict__ w, const int *__restrict__ mem, int nmem,
                                                            int ngl, double *__restrict__ part) {
  __shared__ double s_p[RG_BS];
  const int tid = threadIdx.x, P = ngl * ngl, EPB = RG_BS / P;
  const int ngroups = (nmem + EPB - 1) / EPB;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int s0 = grp * EPB;
    const int nel = min(EPB, nmem - s0);
    if (tid < nel * P) {
      const int le = tid / P;
      s_p[tid] = w[(size_t)mem[s0 + le] * P + (tid - le * P)] * 1.0;
    }
    __syncthreads();
    if (tid < nel) {
      const double *s = s_p + tid * P;
      double sum = s[0];
      for (int n = 1; n < P; n++) sum = sum + s[n];
      part[s0 + tid] = sum;
    }
    __syncthreads();
  }
}

// One pass of the segmented tree.  Workgroup (c, row) reduces descriptor c of the pass (region_plan.h:
// x = input start, y = count <= RG_CHUNK, z = output index, w = final?) of row `row` of `in` (nin values
// per row) by the halving of stats_tree_kernel, and writes the value to the next level (nout values per
// row) or, for a region that is down to one value, to slot z of the series entry [V][R].  Count 0: an
// empty region, +0.0.  The number of workgroups is the number of descriptors: every region of the set in
// one launch.
__global__ void __launch_bounds__(RG_BS) region_tree_kernel(const int4 *__restrict__ desc, const double *__restrict__ in, size_t nin,
                                                            double *__restrict__ next, size_t nout, double *__restrict__ entry,
                                                            int R) {
  __shared__ double x[RG_CHUNK];
  const int tid = threadIdx.x, row = blockIdx.y;
  const int4 d = desc[blockIdx.x];
  const double *p = in + (size_t)row * nin + d.x;
  for (int i = tid; i < d.y; i += RG_BS) x[i] = p[i];
  tree_halve(x, d.y, tid);
  if (tid == 0) {
    const double v = d.y > 0 ? x[0] : 0.0;
    if (d.w)
      entry[(size_t)row * R + d.z] = v;
    else
      next[(size_t)row * nout + d.z] = v;
  }
}

}  // namespace hnumo
