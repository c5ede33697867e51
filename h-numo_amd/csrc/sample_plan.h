// sample_plan.h -- the host-only plan of a sample set (hnumo_sample_create, hnumo_sample_create_ref).
//
// Plain C++17, no HIP call: engine.hip includes it for the engine, tests/sample_plan_main.cpp for a
// CPU program that runs under the host sanitizers (tests/test_sample_plan.py).
//
// A sample set is M points, each a 1-based local element (0: not on this rank) and reference
// coordinates (xi, eta) in [-1,1]^2.  The plan
//   * locates physical points xy(2,M) in the rank's OWNED elements (sample_locate): the elements are
//     straight-sided bilinear quadrilaterals, whose map is inverted with Newton from the four corner
//     nodes; candidates come from a uniform bucket grid over the element bounding boxes; an element
//     accepts a point when max(|xi|, |eta|) <= 1 + tol_e, the lowest accepting element wins, and
//     (xi, eta) are then clamped to [-1,1].  tol_e = 64 eps max|coord| / (half the element's shortest
//     edge): the bilinear map is evaluated with a handful of roundings of magnitude max|coord|, a
//     floor Newton cannot get under, and 64 leaves about a factor of 8;
//   * or takes (elem, xi, eta) as the caller gives them (sample_take_ref);
//   * forms the 1-D Lagrange weights Lx[i] = l_i(xi), Ly[j] = l_j(eta) on the LGL nodes xgl
//     (sample_weights: w = 1; for m != i in ascending order: w = w * ((x - xgl[m]) / (xgl[i] - xgl[m]))
//     -- each factor a quotient first);
//   * and builds the kernel's work lists (sample_chunks): the points sorted stably by element, cut
//     into chunks of at most SP_CHUNK points that touch at most K distinct elements (K: what the
//     kernel's LDS arena holds, sp_K), per chunk the distinct elements and per point its element
//     slot, and the permutation back to input order.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

namespace hnumo {

constexpr int SP_CHUNK = 256;          // points per chunk = lanes of the kernel's workgroup
constexpr int SP_LDS_BYTES = 32768;    // the kernel's LDS arena: five workgroups per CU
constexpr int SP_MAXSETS = 8;
constexpr int SP_SRC_STATE = 0, SP_SRC_STATS = 1;   // HNUMO_SAMPLE_STATE, HNUMO_SAMPLE_STATS
constexpr int SP_SRC_VORT = 2;                      // HNUMO_SAMPLE_VORT
constexpr int SP_SRC_COV = 3;                       // HNUMO_SAMPLE_COV
constexpr int SP_ERR_INVALID = 4;                   // HNUMO_ERR_INVALID

// values per point, doubles per element in the arena (an odd count: consecutive element slots
// start on different LDS banks) and the element slots K of the arena
constexpr int sp_nval(int L, int source) {
  return source == SP_SRC_COV ? 16 * L : source == SP_SRC_VORT ? 4 * L : source == SP_SRC_STATS ? 5 * L : 5 * L + 4;
}
constexpr int sp_estride(int ngl, int V) { return (V * ngl * ngl) | 1; }
constexpr int sp_K(int ngl, int V) { return SP_LDS_BYTES / (8 * sp_estride(ngl, V)); }

struct SamplePlan {
  int ngl = 0, K = 0;
  int64_t M = 0;
  double maxc = 0.0;                   // max |coord| over x, y of the owned nodes (located sets)
  std::vector<int32_t> elem;           // [M] 1-based local element, 0 = none (input order)
  std::vector<double> xi_eta;          // (2,M) (input order)
  // the kernel's tables, in sorted order s = 0..M-1
  std::vector<int32_t> perm;           // [M] input position of sorted point s
  std::vector<int32_t> slot;           // [M] element slot within the point's chunk, -1 = no element
  std::vector<double> w;               // [2 ngl][M] planar: rows 0..ngl-1 Lx, ngl..2ngl-1 Ly
  std::vector<int32_t> chunk_pt;       // [nchunks+1] first sorted point of each chunk
  std::vector<int32_t> chunk_el;       // [nchunks+1] first entry of each chunk in el_list
  std::vector<int32_t> el_list;        // 0-based distinct elements, chunk after chunk
  int nchunks() const { return (int)chunk_pt.size() - 1; }
};

inline int sample_check_xgl(const double *xgl, int ngl, const char *who, std::string &err) {
  if (!xgl) return err = std::string(who) + ": xgl is NULL", SP_ERR_INVALID;
  bool ok = ngl >= 2 && xgl[0] == -1.0 && xgl[ngl - 1] == 1.0;
  for (int i = 1; ok && i < ngl; i++) ok = xgl[i] > xgl[i - 1];   // (false for a NaN)
  if (!ok) return err = std::string(who) + ": xgl must ascend strictly from -1 to 1", SP_ERR_INVALID;
  return 0;
}

// l_i(x), i = 0..ngl-1, into out[i * stride]
inline void sample_weights(const double *xgl, int ngl, double x, double *out, size_t stride) {
  for (int i = 0; i < ngl; i++) {
    double w = 1.0;
    for (int m = 0; m < ngl; m++)
      if (m != i) w = w * ((x - xgl[m]) / (xgl[i] - xgl[m]));
    out[(size_t)i * stride] = w;
  }
}

// the bilinear map of an element's corners c[4][2] (counter-clockwise from (-1,-1)) and its Jacobian
inline void sample_bilinear(const double (&c)[4][2], double xi, double eta, double (&x)[2], double (*J)[2] = nullptr) {
  const double w[4] = {0.25 * (1 - xi) * (1 - eta), 0.25 * (1 + xi) * (1 - eta), 0.25 * (1 + xi) * (1 + eta),
                       0.25 * (1 - xi) * (1 + eta)};
  for (int d = 0; d < 2; d++) x[d] = w[0] * c[0][d] + w[1] * c[1][d] + w[2] * c[2][d] + w[3] * c[3][d];
  if (J)
    for (int d = 0; d < 2; d++) {
      J[d][0] = 0.25 * (-(1 - eta) * c[0][d] + (1 - eta) * c[1][d] + (1 + eta) * c[2][d] - (1 + eta) * c[3][d]);
      J[d][1] = 0.25 * (-(1 - xi) * c[0][d] - (1 + xi) * c[1][d] + (1 + xi) * c[2][d] + (1 - xi) * c[3][d]);
    }
}

inline void sample_corners(const double *coord, int ldc, int ngl, int e, double (&c)[4][2]) {
  const size_t n0 = (size_t)e * ngl * ngl;
  const size_t nd[4] = {n0, n0 + (size_t)ngl - 1, n0 + (size_t)ngl * ngl - 1, n0 + (size_t)ngl * (ngl - 1)};
  for (int m = 0; m < 4; m++)
    for (int d = 0; d < 2; d++) c[m][d] = coord[(size_t)ldc * nd[m] + d];
}

// Newton on the bilinear map from the element centre; false: no finite solution
inline bool sample_invert(const double (&c)[4][2], double px, double py, double &xi, double &eta) {
  xi = eta = 0.0;
  for (int it = 0; it < 32; it++) {
    double x[2], J[2][2];
    sample_bilinear(c, xi, eta, x, J);
    const double rx = px - x[0], ry = py - x[1];
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double dxi = (J[1][1] * rx - J[0][1] * ry) / det, deta = (J[0][0] * ry - J[1][0] * rx) / det;
    if (!std::isfinite(dxi) || !std::isfinite(deta)) return false;
    xi += dxi;
    eta += deta;
    if (std::fabs(xi) > 1e3 || std::fabs(eta) > 1e3) return false;   // far outside: not this element's point
    if (std::fabs(dxi) <= 1e-16 && std::fabs(deta) <= 1e-16) break;
  }
  return true;
}

// Location of xy(2,M) in the owned elements.  Fills p.M, p.ngl, p.maxc, p.elem, p.xi_eta.
inline int sample_locate(const double *coord, int ldc, const double *xgl, int ngl, int nelem_owned, const double *xy,
                         int64_t M, SamplePlan &p, std::string &err, const char *who = "hnumo_sample_create") {
  if (!coord) return err = std::string(who) + ": coord is NULL", SP_ERR_INVALID;
  if (!xy) return err = std::string(who) + ": xy is NULL", SP_ERR_INVALID;
  if (ldc != 2 && ldc != 3)
    return err = std::string(who) + ": ldc must be 2 or 3 (coord(ldc,npoin)), got " + std::to_string(ldc), SP_ERR_INVALID;
  if (M < 1 || M > (int64_t)std::numeric_limits<int32_t>::max())
    return err = std::string(who) + ": M must be >= 1 (and < 2^31), got " + std::to_string(M), SP_ERR_INVALID;
  if (int rc = sample_check_xgl(xgl, ngl, who, err)) return rc;
  const int ne = nelem_owned, P = ngl * ngl;
  const double eps = std::numeric_limits<double>::epsilon();
  double maxc = 0.0;
  for (size_t I = 0; I < (size_t)ne * P; I++)
    for (int d = 0; d < 2; d++) {
      const double v = std::fabs(coord[ldc * I + d]);
      if (!(v <= std::numeric_limits<double>::max()))
        return err = std::string(who) + ": coord is not finite at node " + std::to_string(I + 1), SP_ERR_INVALID;
      maxc = std::max(maxc, v);
    }
  const double tol_x = 64.0 * eps * maxc;
  // per element: corners, bounding box (padded by what tol_e is worth in x, y), tol_e; and the
  // contract: every node is the bilinear map of the corners at (xgl(i), xgl(j))
  struct El {
    double c[4][2], lo[2], hi[2], tol;
  };
  std::vector<El> el(ne);
  double glo[2] = {INFINITY, INFINITY}, ghi[2] = {-INFINITY, -INFINITY};
  for (int e = 0; e < ne; e++) {
    El &E = el[e];
    sample_corners(coord, ldc, ngl, e, E.c);
    for (int j = 0; j < ngl; j++)
      for (int i = 0; i < ngl; i++) {
        double x[2];
        sample_bilinear(E.c, xgl[i], xgl[j], x);
        const size_t I = (size_t)e * P + (size_t)j * ngl + i;
        if (!(std::fabs(x[0] - coord[ldc * I]) <= tol_x) || !(std::fabs(x[1] - coord[ldc * I + 1]) <= tol_x))
          return err = std::string(who) + ": element " + std::to_string(e + 1) + " is not the bilinear map of its corners at node (" +
                       std::to_string(i + 1) + "," + std::to_string(j + 1) + "): curved elements are not supported",
                 SP_ERR_INVALID;
      }
    double smin = INFINITY, diag = 0.0;
    for (int d = 0; d < 2; d++) E.lo[d] = INFINITY, E.hi[d] = -INFINITY;
    for (int m = 0; m < 4; m++) {
      const double ex = E.c[(m + 1) & 3][0] - E.c[m][0], ey = E.c[(m + 1) & 3][1] - E.c[m][1];
      smin = std::min(smin, std::sqrt(ex * ex + ey * ey));
      for (int d = 0; d < 2; d++) E.lo[d] = std::min(E.lo[d], E.c[m][d]), E.hi[d] = std::max(E.hi[d], E.c[m][d]);
    }
    if (!(smin > 0.0))
      return err = std::string(who) + ": element " + std::to_string(e + 1) + " has an edge of length 0", SP_ERR_INVALID;
    E.tol = tol_x / (0.5 * smin);
    diag = (E.hi[0] - E.lo[0]) + (E.hi[1] - E.lo[1]);
    const double pad = 2.0 * (E.tol * diag + tol_x);   // |dX/dxi| <= half the longest edge <= diag
    for (int d = 0; d < 2; d++) {
      E.lo[d] -= pad, E.hi[d] += pad;
      glo[d] = std::min(glo[d], E.lo[d]), ghi[d] = std::max(ghi[d], E.hi[d]);
    }
  }
  // the bucket grid: about one element per bucket; an element is listed (in ascending order) in
  // every bucket its padded box overlaps.  bucket() is monotone, so a point inside a box lies in a
  // bucket between those of the box's ends.
  int nb[2] = {1, 1};
  double bw[2] = {1.0, 1.0};
  if (ne > 0) {
    const int n1 = std::max(1, std::min(4096, (int)std::ceil(std::sqrt((double)ne))));
    for (int d = 0; d < 2; d++) {
      nb[d] = n1;
      bw[d] = (ghi[d] - glo[d]) / n1;
      if (!(bw[d] > 0.0)) nb[d] = 1, bw[d] = 1.0;
    }
  }
  auto bucket = [&](double x, int d) {
    const double t = std::floor((x - glo[d]) / bw[d]);
    return t < 0.0 ? 0 : t >= (double)nb[d] ? nb[d] - 1 : (int)t;
  };
  std::vector<int32_t> bstart((size_t)nb[0] * nb[1] + 1, 0), blist;
  for (int pass = 0; pass < 2; pass++) {
    for (int e = 0; e < ne; e++) {
      const int x0 = bucket(el[e].lo[0], 0), x1 = bucket(el[e].hi[0], 0), y0 = bucket(el[e].lo[1], 1), y1 = bucket(el[e].hi[1], 1);
      for (int by = y0; by <= y1; by++)
        for (int bx = x0; bx <= x1; bx++) {
          const size_t b = (size_t)by * nb[0] + bx;
          if (pass == 0)
            bstart[b + 1]++;
          else
            blist[bstart[b]++] = e;
        }
    }
    if (pass == 0) {
      for (size_t b = 0; b < (size_t)nb[0] * nb[1]; b++) bstart[b + 1] += bstart[b];
      blist.resize(bstart.back());
    } else {
      for (size_t b = (size_t)nb[0] * nb[1]; b > 0; b--) bstart[b] = bstart[b - 1];
      bstart[0] = 0;
    }
  }
  p.M = M;
  p.ngl = ngl;
  p.maxc = maxc;
  p.elem.assign(M, 0);
  p.xi_eta.assign(2 * (size_t)M, 0.0);
  for (int64_t m = 0; m < M; m++) {
    const double px = xy[2 * m], py = xy[2 * m + 1];
    if (!std::isfinite(px) || !std::isfinite(py) || ne == 0) continue;
    if (px < glo[0] || px > ghi[0] || py < glo[1] || py > ghi[1]) continue;
    const size_t b = (size_t)bucket(py, 1) * nb[0] + bucket(px, 0);
    for (int32_t t = bstart[b]; t < bstart[b + 1]; t++) {
      const int e = blist[t];
      const El &E = el[e];
      if (px < E.lo[0] || px > E.hi[0] || py < E.lo[1] || py > E.hi[1]) continue;
      double xi, eta;
      if (!sample_invert(E.c, px, py, xi, eta)) continue;
      if (!(std::max(std::fabs(xi), std::fabs(eta)) <= 1.0 + E.tol)) continue;
      p.elem[m] = e + 1;
      p.xi_eta[2 * m] = std::min(1.0, std::max(-1.0, xi));
      p.xi_eta[2 * m + 1] = std::min(1.0, std::max(-1.0, eta));
      break;
    }
  }
  return 0;
}

// The caller's own location.  Fills p.M, p.ngl, p.elem, p.xi_eta.
inline int sample_take_ref(const double *xgl, int ngl, int nelem_owned, const int32_t *elem, const double *xi_eta, int64_t M,
                           SamplePlan &p, std::string &err) {
  const char *who = "hnumo_sample_create_ref";
  if (!elem) return err = std::string(who) + ": elem is NULL", SP_ERR_INVALID;
  if (!xi_eta) return err = std::string(who) + ": xi_eta is NULL", SP_ERR_INVALID;
  if (M < 1 || M > (int64_t)std::numeric_limits<int32_t>::max())
    return err = std::string(who) + ": M must be >= 1 (and < 2^31), got " + std::to_string(M), SP_ERR_INVALID;
  if (int rc = sample_check_xgl(xgl, ngl, who, err)) return rc;
  for (int64_t m = 0; m < M; m++) {
    if (elem[m] < 0 || elem[m] > nelem_owned)
      return err = std::string(who) + ": elem(" + std::to_string(m + 1) + ") = " + std::to_string(elem[m]) +
                   " is outside 0.." + std::to_string(nelem_owned) + " (the owned elements; 0: not on this rank)",
             SP_ERR_INVALID;
    for (int d = 0; d < 2; d++)
      if (!(std::fabs(xi_eta[2 * m + d]) <= 1.0))   // (false for a NaN)
        return err = std::string(who) + ": xi_eta(" + std::to_string(d + 1) + "," + std::to_string(m + 1) +
                     ") is outside [-1,1] or not finite",
               SP_ERR_INVALID;
  }
  p.M = M;
  p.ngl = ngl;
  p.elem.assign(elem, elem + M);
  p.xi_eta.assign(xi_eta, xi_eta + 2 * M);
  return 0;
}

// The kernel's tables from p.elem, p.xi_eta: weights, sorted order, chunks of at most SP_CHUNK points
// and K distinct elements.
inline void sample_chunks(const double *xgl, int K, SamplePlan &p) {
  const int64_t M = p.M;
  const int ngl = p.ngl;
  p.K = K;
  p.perm.resize(M);
  for (int64_t m = 0; m < M; m++) p.perm[m] = (int32_t)m;
  std::stable_sort(p.perm.begin(), p.perm.end(), [&](int32_t a, int32_t b) { return p.elem[a] < p.elem[b]; });
  p.slot.assign(M, -1);
  p.w.assign((size_t)2 * ngl * M, 0.0);
  p.chunk_pt.assign(1, 0);
  p.chunk_el.assign(1, 0);
  p.el_list.clear();
  int npts = 0, nel = 0, last = 0;   // of the open chunk; last: its latest element (1-based), 0 none
  for (int64_t s = 0; s < M; s++) {
    const int64_t m = p.perm[s];
    const int e = p.elem[m];
    const bool fresh = e != 0 && e != last;
    if (npts == SP_CHUNK || (fresh && nel == K)) {
      p.chunk_pt.push_back((int32_t)s);
      p.chunk_el.push_back((int32_t)p.el_list.size());
      npts = nel = last = 0;
    }
    if (e != 0) {
      if (e != last) {
        p.el_list.push_back(e - 1);
        nel++;
        last = e;
      }
      p.slot[s] = nel - 1;
      sample_weights(xgl, ngl, p.xi_eta[2 * m], &p.w[s], (size_t)M);
      sample_weights(xgl, ngl, p.xi_eta[2 * m + 1], &p.w[(size_t)ngl * M + s], (size_t)M);
    }
    npts++;
  }
  p.chunk_pt.push_back((int32_t)M);
  p.chunk_el.push_back((int32_t)p.el_list.size());
}

}  // namespace hnumo
