// region_plan.h -- the host-only plan of a region set (hnumo_regions_create).
//
// Plain C++17, no HIP call: engine.hip includes it for the engine, tests/region_plan_main.cpp for a
// CPU program that runs under the host sanitizers (tests/test_region_plan.py).
//
// Definitions (normative; include/hnumo_engine.h, DESIGN.md §6.1.9, kernels_region.hip,
// hnumo/regions.py).  A region set labels every owned element with a region r in 0..R; label 0: the
// element is in no region.  Up to RG_MAXSETS sets exist at once (overlapping partitions, such as strips
// and basins, are separate sets).  The members of region r, in ascending local element number, have
// local positions 0..n_r-1.  IEEE double, -ffp-contract=off: no FMA; IEEE division; every sum left to
// right from its first product.  Per member element e, layer k, node I = e*P + j*ngl + i, w_I the nodal
// jac (NS_W):
//   FLOW rows (mask bit 0), the statements of §6.1.1:
//     dp = q(1); h = (alpha_k/gravity)*dp; u = q(2)/dp; v = q(3)/dp
//     VOL_k = int h;  TU_k = int (u*h);  TV_k = int (v*h);  KE_k = int ((0.5*(u*u+v*v))*h)
//   VORT rows (mask bit 1), the statements of §6.1.4 through vort_node; f the caller's coriolis_df, 0
//   for NULL:
//     Z_k = int ((0.5*(zeta*zeta))*h);  PZ_k = int ((0.5*(pv*pv))*h);  G_k = int zeta
// `int` in two steps: per element the products w_I*x_I added in node order from the first product; per
// region the element sums combined by §6.1.1's pairwise tree over the LOCAL POSITIONS (entry i of the
// next level is x[2i] + x[2i+1], or x[2i] alone where 2i+1 does not exist).  An empty region reads +0.0
// in every row.  No floating-point atomics.  Ghost elements are never members.
// Entry: (V, R), V = 4L*[FLOW] + 3L*[VORT]; FLOW rows first, 4(k-1) + {0 VOL, 1 TU, 2 TV, 3 KE}, then the
// VORT rows, 3(k-1) + {0 Z, 1 PZ, 2 G} (hnumo_vort_series' order).  A set whose only region holds all
// owned elements has local position = element position: its KE_k, VOL_k are the bits of
// hnumo_stats_series, its Z_k, PZ_k, G_k those of hnumo_vort_series.
//
// The plan
//   * validates, in this order: region_of_elem NULL; nregions < 1; n != nelem_owned; rows_mask empty or
//     with bits beyond the two; a label outside 0..nregions (the first such element is named);
//   * builds the member list sorted by (region, element), slot[e] (the member's position in that list,
//     -1 for a non-member) and the region offsets;
//   * and per tree pass the chunk descriptors (input start, count <= RG_CHUNK, output index, final?):
//     the chunks of pass 0 are the aligned RG_CHUNK-blocks of each region's local positions; pass p+1
//     runs over each unfinished region's ceil(n/RG_CHUNK) results of pass p, which lie side by side in
//     that pass' output.  A region that is down to one value is final: the value goes to slot r-1 of the
//     series entry, and no later pass touches the region.  An empty region gets one descriptor of count
//     0 in pass 0: a zero write.  The aligned power-of-two blocks of a position-defined tree give the
//     bits of the whole tree, so the passes are the tree of the definition.
// region_tree_host walks the same descriptors on host doubles.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace hnumo {

constexpr int RG_MAXSETS = 4;           // HNUMO_REGION_MAXSETS
constexpr int RG_CHUNK = 1024;          // values per descriptor: ST_CHUNK (kernels_stats.hip), a power of two
constexpr int RG_FLOW = 1, RG_VORT = 2; // HNUMO_REGION_FLOW, HNUMO_REGION_VORT
constexpr int RG_ERR_INVALID = 4;       // HNUMO_ERR_INVALID

// rows of an entry, and the first VORT row
constexpr int rg_rows(int L, int mask) { return (mask & RG_FLOW ? 4 * L : 0) + (mask & RG_VORT ? 3 * L : 0); }
constexpr int rg_vort_base(int L, int mask) { return mask & RG_FLOW ? 4 * L : 0; }

struct RegionChunk {
  int32_t start, count, out, final;     // input start, values (<= RG_CHUNK; 0: a zero write), output index, to the entry?
};

struct RegionPass {
  int64_t nin = 0, nout = 0;            // values per row of the pass' input and of its output level (0: none)
  std::vector<RegionChunk> chunks;
};

struct RegionPlan {
  int R = 0, mask = 0;
  int64_t ne = 0;
  std::vector<int32_t> members;         // 0-based elements, sorted by (region, element)
  std::vector<int32_t> slot;            // [ne] position in members, -1: in no region
  std::vector<int32_t> offset;          // [R+1] region r's members are members[offset[r-1] .. offset[r])
  std::vector<RegionPass> pass;         // at least one
  int64_t nmem() const { return (int64_t)members.size(); }
  int64_t count(int r) const { return offset[r] - offset[r - 1]; }
  // values per row the two level buffers must hold (pass p writes level p & 1)
  int64_t level_size(int b) const {
    int64_t n = 1;
    for (size_t p = b; p < pass.size(); p += 2) n = std::max(n, pass[p].nout);
    return n;
  }
};

inline int region_plan(const int32_t *region_of_elem, int64_t n, int32_t nregions, int32_t rows_mask, int64_t nelem_owned,
                       RegionPlan &pl, std::string &err, const char *who = "hnumo_regions_create") {
  const std::string w = std::string(who) + ": ";
  if (!region_of_elem) return err = w + "region_of_elem is NULL", RG_ERR_INVALID;
  if (nregions < 1) return err = w + "nregions must be >= 1, got " + std::to_string(nregions), RG_ERR_INVALID;
  if (n != nelem_owned)
    return err = w + "n must be nelem_owned = " + std::to_string(nelem_owned) + ", got " + std::to_string(n), RG_ERR_INVALID;
  if (rows_mask == 0 || (rows_mask & ~(RG_FLOW | RG_VORT)))
    return err = w + "rows_mask must hold HNUMO_REGION_FLOW (1), HNUMO_REGION_VORT (2) or both, got " +
                 std::to_string(rows_mask), RG_ERR_INVALID;
  for (int64_t e = 0; e < n; e++)
    if (region_of_elem[e] < 0 || region_of_elem[e] > nregions)
      return err = w + "region_of_elem(" + std::to_string(e + 1) + ") = " + std::to_string(region_of_elem[e]) +
                   " is outside 0.." + std::to_string(nregions), RG_ERR_INVALID;
  pl = RegionPlan{};
  const int R = pl.R = nregions;
  pl.mask = rows_mask;
  pl.ne = n;
  // counting sort by region: ascending element number within a region
  pl.offset.assign((size_t)R + 1, 0);
  for (int64_t e = 0; e < n; e++)
    if (region_of_elem[e] > 0) pl.offset[region_of_elem[e]]++;
  for (int r = 1; r <= R; r++) pl.offset[r] += pl.offset[r - 1];
  pl.members.assign((size_t)pl.offset[R], 0);
  pl.slot.assign((size_t)n, -1);
  {
    std::vector<int32_t> next(pl.offset.begin(), pl.offset.end() - 1);
    for (int64_t e = 0; e < n; e++)
      if (const int r = region_of_elem[e]; r > 0) {
        pl.slot[e] = next[r - 1]++;
        pl.members[pl.slot[e]] = (int32_t)e;
      }
  }
  // the passes: cur[r] = (start, count) of region r's values in the pass' input, count 0: finished
  struct Span {
    int64_t start, count;
  };
  std::vector<Span> cur((size_t)R);
  for (int r = 1; r <= R; r++) cur[r - 1] = Span{pl.offset[r - 1], pl.count(r)};
  int64_t nin = pl.nmem();
  for (bool first = true;; first = false) {
    RegionPass ps;
    ps.nin = nin;
    int64_t nout = 0;
    bool more = false;
    for (int r = 0; r < R; r++) {
      Span &s = cur[r];
      if (s.count == 0) {
        if (first) ps.chunks.push_back(RegionChunk{0, 0, r, 1});   // an empty region: +0.0
        continue;
      }
      const int64_t nch = (s.count + RG_CHUNK - 1) / RG_CHUNK;
      const bool fin = nch == 1;
      for (int64_t c = 0; c < nch; c++)
        ps.chunks.push_back(RegionChunk{(int32_t)(s.start + c * RG_CHUNK), (int32_t)std::min<int64_t>(RG_CHUNK, s.count - c * RG_CHUNK),
                                        fin ? r : (int32_t)(nout + c), fin ? 1 : 0});
      s = fin ? Span{0, 0} : Span{nout, nch};
      if (!fin) nout += nch, more = true;
    }
    ps.nout = nout;
    pl.pass.push_back(std::move(ps));
    if (!more) break;
    nin = nout;
  }
  return 0;
}

// One descriptor's chunk of x[0..m) by the halving of stats_tree_kernel: level after level, entry i of the
// next level is x[2i] + x[2i+1], or x[2i] alone.  In place (entry i is written after 2i and 2i+1 are read).
inline double region_chunk_host(double *x, int m) {
  if (m == 0) return 0.0;
  while (m > 1) {
    const int h = (m + 1) >> 1;
    for (int i = 0; i < h; i++) x[i] = 2 * i + 1 < m ? x[2 * i] + x[2 * i + 1] : x[2 * i];
    m = h;
  }
  return x[0];
}

// The passes of the plan on host doubles: part [rows][nmem] -> entry [rows][R]
inline void region_tree_host(const RegionPlan &pl, int rows, const double *part, double *entry) {
  std::vector<double> lvl[2], x(RG_CHUNK);
  for (int b = 0; b < 2; b++) lvl[b].assign((size_t)rows * pl.level_size(b), 0.0);
  const double *in = part;
  for (size_t p = 0; p < pl.pass.size(); p++) {
    const RegionPass &ps = pl.pass[p];
    double *next = lvl[p & 1].data();
    for (int row = 0; row < rows; row++)
      for (const RegionChunk &c : ps.chunks) {
        for (int i = 0; i < c.count; i++) x[i] = in[(size_t)row * ps.nin + c.start + i];
        const double v = region_chunk_host(x.data(), c.count);
        if (c.final)
          entry[(size_t)row * pl.R + c.out] = v;
        else
          next[(size_t)row * ps.nout + c.out] = v;
      }
    in = next;
  }
}

}  // namespace hnumo
