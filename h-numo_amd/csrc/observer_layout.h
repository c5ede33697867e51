// observer_layout.h -- the host-only index work of the observers (observers.hip): the paired sums between
// the device's layout and the caller's, the transpose of planar entries, the launch grid of a kernel that
// walks items in groups.  Plain C++ with no HIP in it: tests/observer_layout_main.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>

namespace hnumo {

// the pair p (two running sums) of layer k at node I in the device's [L][NP][npoin] pairs: st_pair
// (kernels_stats.hip) at NP = 2, cv_pair (kernels_cov.hip) at NP = CV_NPAIR
inline size_t pair_index(int NP, int k, int p, size_t I, size_t npoin) { return ((size_t)k * NP + p) * npoin + I; }

// the device's [L][NP][npoin][2] -> the caller's (2*NP,npoin,L), and back
inline void pairs_unpack(const double *raw, int NP, int L, size_t npoin, double *out) {
  for (int k = 0; k < L; k++)
    for (int p = 0; p < NP; p++)
      for (size_t I = 0; I < npoin; I++)
        for (int j = 0; j < 2; j++) out[2 * NP * (I + npoin * k) + 2 * p + j] = raw[2 * pair_index(NP, k, p, I, npoin) + j];
}

inline void pairs_pack(const double *in, int NP, int L, size_t npoin, double *raw) {
  for (int k = 0; k < L; k++)
    for (int p = 0; p < NP; p++)
      for (size_t I = 0; I < npoin; I++)
        for (int j = 0; j < 2; j++) raw[2 * pair_index(NP, k, p, I, npoin) + j] = in[2 * NP * (I + npoin * k) + 2 * p + j];
}

// planar [V][M] entries -> the caller's (V,M[,count])
inline void sample_transpose(const double *raw, int V, size_t M, size_t count, double *out) {
  for (size_t c = 0; c < count; c++)
    for (int v = 0; v < V; v++) {
      const double *r = raw + (c * V + v) * M;
      double *o = out + c * V * M + v;
      for (size_t m = 0; m < M; m++) o[m * V] = r[m];
    }
}

// the workgroups of a kernel whose workgroup takes `per` of the n items at a time and goes on in strides of
// the grid: one per group, at least 1, at most `most`
inline int block_count(size_t n, size_t per, size_t most = 8192) {
  return (int)std::max<size_t>(1, std::min<size_t>((n + per - 1) / per, most));
}

}  // namespace hnumo
