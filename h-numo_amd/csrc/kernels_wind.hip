// kernels_wind.hip -- the wind stress as a linear combination of M patterns, formed on the device
// into all four homes the engine keeps it in (hnumo_wind_*, include/hnumo_engine.h).
//
// Arithmetic (normative).  Patterns T_m(2,npoin_q), m = 0..M-1, coefficients
// c_0..c_{M-1}; for each component and quad point
//
//   tau = c_0*T_0;  for m = 1..M-1: tau = tau + c_m*T_m       (left to right, product first)
//   s = 0.0;  N_btp times: s = s + tau;  ave = s / double(N_btp)
//
// the second line being btp_finalize_kernel's statement (mod_rk_mlswe.F90:117,129): the persistent
// sub-cycle never re-forms tau_wind_ave, so it is written here with the wind itself.  Built with
// -ffp-contract=off: no FMA.  The host mirror is hnumo/wind.py (blend, ave), equal bit for bit.
//
// One lane per quad point, consecutive lanes on consecutive quad points: the patterns (the caller's
// (2,npoin_q,M) layout) are read and tau_wind, tau_wind_ave written as 16-byte pairs, the rows
// QS_TW1/QS_TW2 of qstat and QE_TW1/QE_TW2 of an element's qstatE record as 8-byte stores contiguous
// across the lanes of the element.  M and NQ are template parameters: the sum is unrolled and the
// element / quad-point split of the lane index divides by a constant.  The coefficients are kernel
// arguments (hnumo_wind_set) or a row of the schedule's device table, read at a wave-uniform address.
// No atomics, no LDS, no barrier; (16 M + 64) npoin_q bytes.
#include "engine_internal.h"

namespace hnumo {

constexpr int WIND_MAXM = 4;
constexpr int WIND_BS = 256;

struct WindArgs {
  const double2 *pat;   // T_m at [m*npq + iq], both components
  const double *row;    // c_0..c_{M-1} on the device, or NULL: c below
  double c[WIND_MAXM];
  double2 *tau, *ave;   // tau_wind(2,npq), tau_wind_ave(2,npq)
  double *qstat;        // [QS_N][npq]
  double *qstatE;       // [E][qe_stride(Q)]
  int npq, N_btp;
};

struct WindCoef {
  double c[WIND_MAXM];
};

// (the pointers are kernel arguments of their own, restrict-qualified: global loads and stores;
// TABLE: the coefficients are the device row's, read through the scalar cache, else the arguments k)
template <int M, int NQ, bool TABLE>
__global__ void __launch_bounds__(WIND_BS)
    wind_blend_kernel(const double2 *__restrict__ pat, const double *__restrict__ row, WindCoef k, double2 *__restrict__ tau,
                      double2 *__restrict__ ave, double *__restrict__ qstat, double *__restrict__ qstatE, int npq_, int N_btp) {
  constexpr unsigned Q = NQ * NQ;
  const unsigned iq = blockIdx.x * WIND_BS + threadIdx.x;
  if (iq >= (unsigned)npq_) return;
  double c[M];
#pragma unroll
  for (int m = 0; m < M; m++) c[m] = TABLE ? row[m] : k.c[m];
  const size_t npq = (size_t)npq_;
  double2 t = pat[iq];
  double t1 = c[0] * t.x, t2 = c[0] * t.y;
#pragma unroll
  for (int m = 1; m < M; m++) {
    t = pat[m * npq + iq];
    t1 = t1 + c[m] * t.x;
    t2 = t2 + c[m] * t.y;
  }
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < N_btp; i++) {
    s1 = s1 + t1;
    s2 = s2 + t2;
  }
  const double nb = (double)N_btp;
  tau[iq] = make_double2(t1, t2);
  ave[iq] = make_double2(s1 / nb, s2 / nb);
  qstat[QS_TW1 * npq + iq] = t1;
  qstat[QS_TW2 * npq + iq] = t2;
  const unsigned e = iq / Q, q = iq - e * Q;
  double *rec = qstatE + (size_t)e * qe_stride(Q);
  rec[qe_pos(QE_TW1, q, Q)] = t1;
  rec[qe_pos(QE_TW2, q, Q)] = t2;
}

#define HNUMO_WIND_LAUNCH(M_)                                                                                      \
  if (a.row)                                                                                                       \
    hipLaunchKernelGGL((wind_blend_kernel<M_, NQ, true>), grid, block, 0, st, a.pat, a.row, k, a.tau, a.ave, a.qstat, \
                       a.qstatE, a.npq, a.N_btp);                                                                  \
  else                                                                                                             \
    hipLaunchKernelGGL((wind_blend_kernel<M_, NQ, false>), grid, block, 0, st, a.pat, a.row, k, a.tau, a.ave, a.qstat, \
                       a.qstatE, a.npq, a.N_btp)

// the launch for M patterns on an NQ x NQ quadrature; false: no such kernel (refused by the caller)
template <int NQ>
static bool wind_launch_m(const WindArgs &a, int M, hipStream_t st) {
  const dim3 grid((unsigned)((a.npq + WIND_BS - 1) / WIND_BS)), block(WIND_BS);
  WindCoef k;
  for (int m = 0; m < WIND_MAXM; m++) k.c[m] = a.c[m];
  switch (M) {
    case 1: HNUMO_WIND_LAUNCH(1); return true;
    case 2: HNUMO_WIND_LAUNCH(2); return true;
    case 3: HNUMO_WIND_LAUNCH(3); return true;
    case 4: HNUMO_WIND_LAUNCH(4); return true;
    default: return false;
  }
}

static bool wind_nq_ok(int nq) { return nq == 5 || nq == 7 || nq == 9 || nq == 11 || nq == 15; }

static bool wind_launch(const WindArgs &a, int M, int nq, hipStream_t st) {
  if (a.npq <= 0) return M >= 1 && M <= WIND_MAXM && wind_nq_ok(nq);
  switch (nq) {
    case 5: return wind_launch_m<5>(a, M, st);
    case 7: return wind_launch_m<7>(a, M, st);
    case 9: return wind_launch_m<9>(a, M, st);
    case 11: return wind_launch_m<11>(a, M, st);
    case 15: return wind_launch_m<15>(a, M, st);
    default: return false;
  }
}

}  // namespace hnumo
