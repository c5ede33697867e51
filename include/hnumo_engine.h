/*
 * hnumo_engine.h -- C ABI of the MI355X DG time-step engine for h-NUMO's multilayer
 * shallow-water (MLSWE) solver.
 *
 * Drop-in boundary.  The reference has no plugin/FFI layer: its hot path is the single
 * Fortran call
 *
 *     call ti_rk_bcl(q0_df_mlswe, qb0_df_mlswe, qprime0_df)     ! mod_time_loop.F90:209
 *
 * (ti_rk_bcl.F90:9-87) with every other input held in module globals (mod_grid,
 * mod_face, mod_basis, mod_metrics, mod_initial, mod_input, mod_constants,
 * mod_variables).  This header replaces that call with
 *
 *     hnumo_engine_create(mesh, statics, params, halo, device, &eng)   -- module globals
 *     hnumo_ti_rk_bcl(eng, q_df, qb_df, qprime_df)                      -- ti_rk_bcl
 *
 * and exposes the two inner entry points as parity hooks:
 *
 *     hnumo_ti_barotropic_ssprk  -- ti_barotropic_ssprk_mlswe (mod_rk_mlswe.F90:19-151)
 *     hnumo_create_rhs_btp       -- create_rhs_btp            (mod_rhs_btp.F90:28-59)
 *
 * Around the step, on the device state and without hnumo_sync: the run diagnostics
 * (hnumo_diagnostics), the online flow statistics -- time means, MKE / EKE, KE series
 * (hnumo_stats_begin .. hnumo_stats_end), sample sets at arbitrary points (hnumo_sample_*) and
 * Lagrangian floats advected with a layer's velocity (hnumo_floats_*).
 *
 * Layout contract.  Every array is the reference's own Fortran (column-major) array,
 * 1-based integers where the reference is 1-based.  The reference's face arrays carry
 * a dead second face index (e.g. normal_vector(3,ngl,ngl,nface) of which only
 * (:,n,1,f) is read on this path); the ABI takes the compacted slice, e.g.
 * normal_vector(:,:,1,:) -> (3,ngl,nface), which a Fortran caller passes as that
 * array section.  Node numbering is the reference's DG convention
 * I = (e-1)*ngl*ngl + (j-1)*ngl + i (intma_dg, mod_grid.F90:230-239); quad numbering
 * Iq = (e-1)*nq*nq + (j-1)*nq + i (intma_dg_quad, :242-250).  Any re-layout is internal.
 *
 * Errors.  The reference `stop`s; the ABI returns a code and keeps the message for
 * hnumo_last_error():
 *   0 OK, 1 negative layer thickness (mod_splitting.F90:74-77,228-231),
 *   2 non-finite value, 3 HIP / RCCL error, 4 invalid argument / unsupported option.
 *
 * Threading.  One host thread per engine, one engine per GPU (rank).  Calls are
 * synchronous on return unless resident mode is on (hnumo_set_resident), in which
 * case state stays on the device between steps and hnumo_sync() copies it out.
 *
 * No torch, HIP or RCCL types appear in this header.
 */
#ifndef HNUMO_ENGINE_H
#define HNUMO_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HNUMO_ABI_VERSION 10

enum {
  HNUMO_OK = 0,
  HNUMO_ERR_NEGATIVE_THICKNESS = 1,
  HNUMO_ERR_NONFINITE = 2,
  HNUMO_ERR_DEVICE = 3,
  HNUMO_ERR_INVALID = 4
};

/* Mesh, basis and metric terms: mod_grid / mod_face / mod_basis / mod_metrics. */
typedef struct hnumo_mesh_desc {
  int32_t nelem, npoin, npoin_q, nface;  /* mod_grid                                  */
  int32_t ngl, nq, nlayers;              /* mod_basis ngl, nq; mod_input nlayers       */
  const int32_t *face;                   /* (8,nface): face(7)=el, face(8)=er | -bc | 0 */
  const int32_t *imapl, *imapr;          /* (3,ngl,nface) = imapl(:,:,1,:)              */
  const double *normal_vector;           /* (3,ngl,nface) = normal_vector(:,:,1,:)      */
  const double *normal_vector_q;         /* (3,nq,nface)  = normal_vector_q(:,:,1,:)    */
  const double *jac_face;                /* (ngl,nface)   = jac_face(:,1,:)             */
  const double *jac_faceq;               /* (nq,nface)    = jac_faceq(:,1,:)            */
  const double *massinv;                 /* (npoin)       mod_metrics                   */
  const double *psiq, *dpsiq;            /* (ngl,nq)      mod_basis                     */
  const double *psi, *dpsi;              /* (ngl,ngl)     mod_basis                     */
  /* per-quad-point metrics (mod_metrics ksiq_x.., jacq = w_i w_j |J|)  (nq,nq,nelem)  */
  const double *ksiq_x, *ksiq_y, *etaq_x, *etaq_y, *jacq;
  /* per-node metrics (ksi_x.., jac = w_i w_j |J|)                      (ngl,ngl,nelem) */
  const double *ksi_x, *ksi_y, *eta_x, *eta_y, *jac;
  /* Optional dense tables of Tensor_product.F90 (mod_initial psih, dpsidx, ...).  Read
   * only by the CPU oracle; the HIP engine ignores them (NULL allowed).             */
  const double *psih, *dpsidx, *dpsidy, *wjac;        /* (npts,npoin_q), wjac (npoin_q) */
  const int32_t *indexq;                              /* (npts,npoin_q)                 */
  const double *dpsidx_df, *dpsidy_df, *wjac_df;      /* (npts,npoin), wjac_df (npoin)  */
  const int32_t *index_df;                            /* (npts,npoin)                   */
  /* face quad point -> element quad point maps, (3,nq,nface) = imapl_q(:,:,1,:)
   * (mod_face, create_normals_quad.F90:335-350); read only when method_visc == 1
   * (quad-point LDG viscosity), NULL allowed otherwise.                              */
  const int32_t *imapl_q, *imapr_q;
} hnumo_mesh_desc;

/* Reference state and forcing built at start-up: mod_initial (mod_initial.F90:42-53). */
typedef struct hnumo_static_desc {
  const double *pbprime;                /* (npoin_q)    */
  const double *pbprime_df;             /* (npoin)      */
  const double *one_over_pbprime;       /* (npoin_q)    */
  const double *one_over_pbprime_df;    /* (npoin)      */
  const double *pbprime_face;           /* (2,nq,nface) */
  const double *pbprime_df_face;        /* (2,ngl,nface)*/
  const double *one_over_pbprime_edge;  /* (nq,nface)   */
  const double *coeff_pbpert_L, *coeff_pbpert_R, *coeff_pbub_LR;            /* (nq,nface) */
  const double *coeff_mass_pbub_L, *coeff_mass_pbub_R, *coeff_mass_pbpert_LR;
  const double *alpha;                  /* (nlayers)  alpha_mlswe = 1/rho_k */
  const double *tau_wind;               /* (2,npoin_q)  */
  const double *coriolis_quad;          /* (npoin_q)    */
  const double *grad_zbot_quad;         /* (2,npoin_q)  */
  const double *zbot_df;                /* (npoin)      */
  const double *zbot_face;              /* (2,nq,nface) */
  const double *fdt2_bcl, *a_bcl, *b_bcl;  /* (npoin)   */
  const double *ssprk_a;                /* (kstages,3)  */
  const double *ssprk_beta;             /* (kstages)    */
} hnumo_static_desc;

/* mod_input / mod_constants scalars used by the path. */
typedef struct hnumo_params {
  double dt, dt_btp;                    /* dt_btp = dt/N_btp (mod_initial.F90:176-177) */
  double visc_mlswe, cd_mlswe, ad_mlswe, gravity;
  int32_t N_btp, kstages, method_visc, botfr;
  /* ad_mlswe > 0 (implicit vertical shear stress, rhs_layer_shear_stress,
   * mod_create_rhs_mlswe.F90:146-279): mod_input max_shear_dz (mod_input.F90:127).      */
  double max_shear_dz;
  /* What the corrector's shear-stress call reads (mod_splitting.F90:158).  The reference
   * passes its never-assigned local `uv` (:119) there; under the reference build's
   * -finit-real=zero (config.user:25) that is all zeros, so dp = 0, the solve divides
   * 0/0 and the corrector's layer momenta become NaN (the engine then returns
   * HNUMO_ERR_NONFINITE).
   *   HNUMO_SHEAR_CORRECTOR_REFERENCE (0, default): exactly that.
   *   HNUMO_SHEAR_CORRECTOR_PREDICTED (1): the Coriolis-rotated, velocity-smoothed
   *     momenta q_df3, as momentum_mass passes them at :265 (the evident intent).       */
  int32_t shear_corrector;
  int32_t reserved;
} hnumo_params;

#define HNUMO_SHEAR_CORRECTOR_REFERENCE 0
#define HNUMO_SHEAR_CORRECTOR_PREDICTED 1

/* Multi-rank description: one of two partition contracts.
 *
 * (1) The reference's own -- PROCESSOR FACES (mod_parallel; p4est.c:1343-1412,1686-1712):
 *     a rank holds only its elements; a face shared with another rank has the local
 *     element as face(7), face(8) = 0, and appears in nbh_send_recv under its neighbour:
 *     num_nbh neighbours with 1-BASED ranks nbh_proc[k], num_send_recv[k] faces each, the
 *     1-based local face ids in an order both ranks agree on, nodes of a shared face listed
 *     in the same physical order on both (as p4est guarantees).  nelem_owned = nelem (or
 *     0); the ghost fields NULL.  The engine exchanges what the reference exchanges
 *     (create_rhs_communicator / send_receive_bound / create_rhs_dynamics_flux): per
 *     barotropic stage the face traces of qb and grad(u_bar) (one message per neighbour,
 *     sent on a second stream while the elements without processor faces run), per
 *     baroclinic step the qprime face traces, graduv_dpp_face and the consistency
 *     deficits.  Results equal the reference Fortran/MPI run on the same partition bit
 *     for bit (tests/test_facehalo_gpu.py).  Non-conforming faces (multiplicity > 1) are
 *     rejected (code 4).
 * (2) A one-element GHOST layer (h-numo_amd/hnumo/partition.py): local elements
 *     1..nelem_owned are owned, nelem_owned+1..nelem are copies of neighbours' elements
 *     whose data the engine refreshes from their owners wherever a kernel reads across an
 *     element boundary; per neighbour k (0-based rank nbh_proc[k]) ghost_send lists the
 *     owned elements that neighbour holds as ghosts, ghost_recv the local ghosts it owns,
 *     in global element order; num_send_recv all 0.  Every owned element's arithmetic is
 *     the single-rank run's, bit for bit.
 *
 * Transport: RCCL point-to-point over xGMI when comm_id (from hnumo_rccl_unique_id,
 * broadcast by the host) is given; engines of one process on one device joined with
 * hnumo_local_group otherwise.  NULL halo or nranks == 1 without lists: single rank.
 * (Test contract: nranks == 1 WITH processor-face lists whose neighbour is the rank itself --
 * each listed face receives its own side 1 -- drives the RCCL code on one GPU.  RCCL across
 * GPUs is verified by bench.py's halo check in a multi-GPU run, INTEGRATION.md.)       */
typedef struct hnumo_halo_desc {
  int32_t rank, nranks;                 /* 0-based rank of this engine, number of ranks */
  int32_t num_nbh;
  const int32_t *nbh_proc;              /* (num_nbh) neighbour ranks (1-based: faces)   */
  const int32_t *num_send_recv;         /* (num_nbh) shared faces per neighbour         */
  const int32_t *nbh_send_recv;         /* (sum num_send_recv) 1-based face ids         */
  const unsigned char *comm_id;         /* 128-byte RCCL unique id (NULL: local group)  */
  int32_t nelem_owned;                  /* owned elements come first                    */
  const int32_t *num_ghost_send;        /* (num_nbh)                                    */
  const int32_t *ghost_send;            /* (sum num_ghost_send) 1-based local elements  */
  const int32_t *num_ghost_recv;        /* (num_nbh)                                    */
  const int32_t *ghost_recv;            /* (sum num_ghost_recv) 1-based local elements  */
} hnumo_halo_desc;

typedef struct hnumo_engine hnumo_engine;   /* opaque: device buffers, streams, graphs */

int  hnumo_engine_create(const hnumo_mesh_desc *mesh, const hnumo_static_desc *statics,
                         const hnumo_params *params, const hnumo_halo_desc *halo,
                         int device, hnumo_engine **out);
void hnumo_engine_destroy(hnumo_engine *eng);
const char *hnumo_last_error(const hnumo_engine *eng);
int  hnumo_abi_version(void);

/* = ti_rk_bcl(q_df, qb_df, qprime_df)  (ti_rk_bcl.F90:9-87)
 *   q_df(3,npoin,nlayers), qb_df(4,npoin), qprime_df(3,npoin,nlayers), all inout.  */
int hnumo_ti_rk_bcl(hnumo_engine *eng, double *q_df, double *qb_df, double *qprime_df);

/* = ti_barotropic_ssprk_mlswe(qb_df, qprime_df) (mod_rk_mlswe.F90:19-151).  Uses the
 *   baroclinic coefficients of the last hnumo_btp_bcl_coeffs / hnumo_ti_rk_bcl call. */
int hnumo_ti_barotropic_ssprk(hnumo_engine *eng, double *qb_df, const double *qprime_df);

/* = btp_bcl_coeffs_qdf(qprime_df_face, qprime_df) with dpprime_visc = qprime_df(1,:,:)
 *   and qprime_df_face from extract_qprime_df_face (ti_rk_bcl.F90:43-50).           */
int hnumo_btp_bcl_coeffs(hnumo_engine *eng, const double *qprime_df);

/* = the prediction half of ti_rk_bcl (ti_rk_bcl.F90:43-57): btp_bcl_coeffs_qdf, the
 *   barotropic sub-cycle, momentum_mass (ABI v6).  In: the step-start state; out: q_df2,
 *   qb_df after the sub-cycle, qprime_df2 (the reference's arrays after :57).  The engine's
 *   device state becomes the caller's input, so a resident engine (hnumo_set_resident)
 *   uploads the caller's arrays again on its next hnumo_ti_rk_bcl (ABI v7).             */
int hnumo_predict(hnumo_engine *eng, double *q_df, double *qb_df, double *qprime_df);

/* = create_rhs_btp(rhs, qb_df, qprime_df) (mod_rhs_btp.F90:28-59); rhs(3,npoin).    */
int hnumo_create_rhs_btp(hnumo_engine *eng, double *rhs, const double *qb_df,
                         const double *qprime_df);

/* Copy out a named engine field (mod_variables equivalents, e.g. "ope_ave", "H_ave",
 * "Qu_face_ave", "graduvb_ave") in the reference's layout; n = element count.       */
int hnumo_get_field(hnumo_engine *eng, const char *name, double *out, int64_t n);

/* Resident mode: state stays on the device across hnumo_ti_rk_bcl calls; the host
 * pointers passed to hnumo_ti_rk_bcl are only read on the first call and written by
 * hnumo_sync().                                                                      */
int hnumo_set_resident(hnumo_engine *eng, int on);
int hnumo_sync(hnumo_engine *eng, double *q_df, double *qb_df, double *qprime_df);

/* Run diagnostics on the device state (additive in ABI v10): what the reference's time loop
 * reports every irestart steps (mod_time_loop.F90:219-254, print_diagnostics.F90:14-190), formed
 * by HIP kernels from q_df and qb_df where they live and returned as a few hundred bytes -- no
 * hnumo_sync.  Every value has the bits the reference's host routines give on the synced state.
 *
 * hnumo_diag_geometry: once per engine (again after the grid moved).  coord(ldc,npoin), ldc = 2
 *   or 3, is mod_grid coord, rows 1-2 are read; wjac_df(npoin) is mod_initial wjac_df, NULL: the
 *   nodal jac of the mesh descriptor (the same numbers).  Builds the running minima of the
 *   sub-cell sizes of courant_cube_mlswe (courant.F90:95-99) -- the reference divides each cell's
 *   velocity by the minimum over the cells up to that one in its loop order, not by the grid's
 *   minimum.  Returns 4 on a NULL coord or another ldc.
 * hnumo_diagnostics: n = 12 + 11*nlayers,
 *   out = [cfl_b, cfl, min_dx, min_dy, qbmax(1:4), qbmin(1:4)], then per layer
 *         [mass, qmax(1:5), qmin(1:5)]
 *   cfl_b, cfl, min_dx, min_dy = courant_cube_mlswe (courant.F90:34-127); qmax/qmin the extrema
 *   over the nodes of h, u, v, dp and the interface elevation (diagnostics.F90:24-45), qbmax/qbmin
 *   those of qb_df (print_diagnostics.F90:60-86); mass = compute_conserved (compute_conserved.F90:
 *   29-41), summed in node order as there.  flags bit 0: include the layer masses (one sequential
 *   chain per layer; clear: the mass slots are 0).  Multi-rank engines report their own elements
 *   (the owned ones of a ghost-layer partition), as each rank of the reference does before its
 *   mpi_reduce; the host combines ranks.  Works on the state on the device: between the steps of
 *   a resident engine, or after the last call of a non-resident one; ordered after the step in
 *   flight on the engine's stream, outside the captured step.  Returns 4 if n is wrong, before
 *   hnumo_diag_geometry, or before any state was uploaded.  Non-finite states are out of contract
 *   (the step returns 2 for them); the sign of an extremum that is exactly zero is unspecified.
 * hnumo_layer_fields: q(5,npoin,nlayers) of diagnostics.F90:24-45 (h, u, v, dp, interface
 *   elevation), the input of the reference's snapshot writers (diagnostics.F90:58-92), computed
 *   on the device; n = 5*npoin*nlayers.                                                      */
#define HNUMO_DIAG_MASS 1
int hnumo_diag_geometry(hnumo_engine *eng, const double *coord, int32_t ldc, const double *wjac_df);
int hnumo_diagnostics(hnumo_engine *eng, int32_t flags, double *out, int64_t n);
int hnumo_layer_fields(hnumo_engine *eng, double *out5, int64_t n);

/* Online flow statistics on the device state (additive in ABI v10): the time means, MKE / EKE and
 * the kinetic-energy series that the double-gyre post-processing (Examples/double_gyre/
 * compute_eke.m, compute_ke.m) forms from hundreds of snapshots, accumulated by HIP kernels where
 * the state lives -- from every step if asked, no hnumo_sync.  Per owned node and layer, from
 * q_df as diagnostics.F90:24-45 forms them: dp = q(1), h = (alpha_k/gravity)*dp, u = q(2)/dp,
 * v = q(3)/dp, uh = u*h, vh = v*h, e = (0.5*(u*u + v*v))*h.  One SAMPLE adds h, uh, vh, e to the
 * running sums S_h, S_uh, S_vh, S_e (plain adds in sample order, from +0.0) and, with a series,
 * appends per layer KE_k = integral of e and VOL_k = integral of h over the rank's owned elements
 * (per element the products jac_I * e_I added in node order; the element sums combined by a
 * pairwise tree over the element positions: fixed bits, no floating-point atomics).  Every value
 * has the bits of the numpy mirror hnumo/flowstats.py (HostFlowStats) on the synced states.
 * Nodes of ghost elements are never accumulated and read 0 in every output.  DESIGN.md §6.1.1.
 *
 * hnumo_stats_begin: allocates and zeroes the sums; a second call resets them.  series_capacity:
 *   samples the series can hold (0: no series, and no reduction work per sample).  every = 0: only
 *   hnumo_stats_accumulate takes samples; every = k >= 1: the engine also takes one itself after
 *   every k-th successful hnumo_ti_rk_bcl (hnumo_group_ti_rk_bcl for grouped engines) since begin,
 *   once the step's abort / retry handling has finished; a step that returns non-zero is not
 *   sampled.  If that sample finds the series full the step call returns 4 (the step is done).
 * hnumo_stats_accumulate: one sample of the state on the device -- between the steps of a resident
 *   engine or after the last call of a non-resident one; ordered after the step on the engine's
 *   stream, outside the captured step, nothing copied back.  The step's launches, graph and bits
 *   are the same with statistics on or off.
 * hnumo_stats_sums / hnumo_stats_set_sums: out / in (4,npoin,nlayers) = S_h, S_uh, S_vh, S_e in the
 *   index order of hnumo_layer_fields, n = 4*npoin*nlayers, and the sample count: a restarted run
 *   restores them and goes on averaging.
 * hnumo_stats_fields: out(5,npoin,nlayers), n = 5*npoin*nlayers, after nsamples samples:
 *   hbar = S_h/nsamples, um = S_uh/S_h, vm = S_vh/S_h, mke = S_e/S_h, eke = mke - 0.5*(um*um + vm*vm).
 * hnumo_stats_series: out(2,nlayers,count) = (KE_k, VOL_k) per sample; n = the doubles out can
 *   hold, at least 2*nlayers*count; out = NULL (n = 0) only returns count.  clear = 1 empties the
 *   series after the copy (the sums stay).  compute_ke.m's per-layer series is KE_k/VOL_k.
 * hnumo_stats_end: frees the buffers; a no-op before hnumo_stats_begin.
 * All return 4, with a message in hnumo_last_error, before hnumo_stats_begin, for a wrong n or
 * negative arguments; a sample returns 4 before any state was uploaded and when the series is full
 * (nothing is accumulated then); hnumo_stats_fields returns 4 with no samples.  Non-finite states
 * are out of contract (the step returns 2 for them).                                          */
int hnumo_stats_begin(hnumo_engine *eng, int32_t every, int32_t series_capacity);
int hnumo_stats_accumulate(hnumo_engine *eng);
int hnumo_stats_sums(hnumo_engine *eng, double *out, int64_t n, int64_t *nsamples);
int hnumo_stats_set_sums(hnumo_engine *eng, const double *in, int64_t n, int64_t nsamples);
int hnumo_stats_fields(hnumo_engine *eng, double *out, int64_t n);
int hnumo_stats_series(hnumo_engine *eng, double *out, int64_t n, int64_t *count, int32_t clear);
int hnumo_stats_end(hnumo_engine *eng);

/* Vorticity products on the device state (additive in ABI v10): relative vorticity, divergence, layer
 * potential vorticity and the Okubo-Weiss parameter, with the enstrophy, potential-enstrophy and
 * circulation series -- the diagnostics an eddying run is judged by, which need the gradient of the
 * layer velocity.  The reference stops short of them (write_output.F90:32,41 allocates `vorticity`
 * and never fills it), so the arithmetic is defined here.  For an owned element e, layer k and node
 * (i, j), I = e*P + j*ngl + i (0-based i, j), every sum left to right from its first product, no FMA:
 *   dp = q(1,I,k);  h = (alpha_k/gravity)*dp (quotient first);  u = q(2,I,k)/dp;  v = q(3,I,k)/dp
 *   D(m,i) = l_m'(xgl_i) (mod_basis dpsi, as the mesh descriptor passes it)
 *   u_xi = sum_m D(m,i)*u(m,j);  u_eta = sum_m D(m,j)*u(i,m)          (v likewise)
 *   u_x = u_xi*ksi_x(I) + u_eta*eta_x(I);  u_y = u_xi*ksi_y(I) + u_eta*eta_y(I)   (v likewise)
 *   zeta = v_x - u_y;  delta = u_x + v_y;  pv = (zeta + f(I))/h
 *   sn = u_x - v_y;  ss = v_x + u_y;  ow = (sn*sn + ss*ss) - zeta*zeta
 * This is the element's own (broken) gradient: no face terms, so no halo and nothing between ranks;
 * jumps at element edges are not lifted.  Series, per sample and layer, over the rank's owned
 * elements: Z_k = integral of (0.5*(zeta*zeta))*h, PZ_k = integral of (0.5*(pv*pv))*h, G_k = integral
 * of zeta, summed exactly as the flow statistics' series (per element the products jac_I * x_I added
 * in node order, the element sums by the pairwise tree over the element positions; the host adds the
 * ranks' entries).  Every value has the bits of the numpy mirror hnumo/vorticity.py (HostVorticity) on
 * the synced state.  Nodes of ghost elements are never formed and read 0.  DESIGN.md §6.1.4.
 *
 * hnumo_vort_begin: coriolis_df(npoin) = mod_initial coriolis_df, or NULL: f = 0.  series_capacity:
 *   samples the series can hold (0: no series).  every = 0: only hnumo_vort_record takes samples;
 *   every = k >= 1: the engine also takes one after every k-th successful hnumo_ti_rk_bcl
 *   (hnumo_group_ti_rk_bcl for grouped engines) since begin, once the step's abort / retry handling
 *   has finished and after the flow statistics' sample, before the sample sets (a VORT set records
 *   the new state) and the floats.  If that sample finds the series full the step call returns 4 (the
 *   step is done).  A second call resets.
 * hnumo_vort_fields: out(4,npoin,nlayers) = zeta, delta, pv, ow in the index order of
 *   hnumo_layer_fields, n = 4*npoin*nlayers, formed now from the state on the device.
 * hnumo_vort_record: appends one series sample on the device; nothing is copied back.
 * hnumo_vort_series: out(3,nlayers,count) = (Z_k, PZ_k, G_k) per sample; n = the doubles out can hold,
 *   at least 3*nlayers*count; out = NULL (n = 0) only returns count.  clear = 1 empties the series
 *   after the copy.
 * hnumo_vort_end: frees the buffers; a no-op before hnumo_vort_begin.
 * All launches are plain launches on the engine stream outside the captured step: the step's
 * launches, graph and bits are the same with or without them.  All return 4, with a message in
 * hnumo_last_error, before hnumo_vort_begin, for a wrong n or negative arguments; a sample returns 4
 * before any state was uploaded and when the series is full or absent.                         */
int hnumo_vort_begin(hnumo_engine *eng, const double *coriolis_df, int32_t every, int32_t series_capacity);
int hnumo_vort_fields(hnumo_engine *eng, double *out, int64_t n);
int hnumo_vort_record(hnumo_engine *eng);
int hnumo_vort_series(hnumo_engine *eng, double *out, int64_t n, int64_t *count, int32_t clear);
int hnumo_vort_end(hnumo_engine *eng);

/* Eddy covariances on the device state (additive in ABI v10): the thickness-weighted Reynolds stress
 * tensor (the EKE is half its trace), the eddy thickness flux (bolus transport), the interface and SSH
 * variance, the eddy potential-vorticity flux and the eddy potential enstrophy -- covariances of fields
 * that decorrelate within a few steps, so they are accumulated from every step where the state lives;
 * the PV terms need the gradient of every sampled state.  Definitions (normative; no FMA, IEEE
 * division, every sum left to right).  Per owned node I of element e and layer k, per sample:
 *   dp, h, u, v        as hnumo_stats / hnumo_vort form them (h = (alpha_k/gravity)*dp, quotient first;
 *                      u = q2/dp; v = q3/dp)
 *   z                  = elevation of layer k's top interface as hnumo_layer_fields forms it (row 5;
 *                        summed upward from zbot_df)
 *   d                  = z - zref(I,k)                  (zref given at begin, NULL: 0.0)
 *   zeta, pv           = zeta and pv of hnumo_vort for this node and layer (f as given at begin, NULL: 0.0)
 *   a                  = zeta + f(I)
 * One SAMPLE adds these 14 terms to running sums (plain adds in sample order from +0.0; one lane owns a
 * node's sums):
 *   S_h  += h        S_u  += u          S_v  += v
 *   S_uh += u*h      S_vh += v*h
 *   S_uuh += (u*u)*h S_uvh += (u*v)*h   S_vvh += (v*v)*h
 *   S_d  += d        S_dd += d*d
 *   S_a  += a        S_ua += u*a        S_va += v*a        S_qa += pv*a
 * zref exists because the top interface of an interior layer sits near -1500 m while its variance is a
 * few m^2: without the shift S_dd/n - dbar^2 loses eight digits.  Pass the rest elevations, or on a
 * restart the zref of the first run.  The fields, 16 per node and layer, after n samples, N = double(n):
 *   hbar = S_h/N   ubar = S_u/N   vbar = S_v/N   um = S_uh/S_h   vm = S_vh/S_h
 *   Ruu = S_uuh/S_h - um*um    Ruv = S_uvh/S_h - um*vm    Rvv = S_vvh/S_h - vm*vm
 *   Fu  = S_uh/N - ubar*hbar   Fv  = S_vh/N - vbar*hbar
 *   dbar = S_d/N               dvar = S_dd/N - dbar*dbar
 *   qm  = S_a/S_h              Qu  = S_ua/S_h - um*qm     Qv = S_va/S_h - vm*qm
 *   ens = 0.5*(S_qa/S_h - qm*qm)
 * Ruu, Ruv, Rvv: the thickness-weighted Reynolds stresses; Fu, Fv: the eddy thickness flux (Fu/hbar is
 * the bolus velocity); dvar of layer 1: the SSH variance; Qu, Qv: the thickness-weighted eddy PV flux
 * (h*pv = a); ens: the eddy potential enstrophy.  Integrals, per layer, over the rank's owned elements:
 * of hbar*(0.5*(Ruu+Rvv)), of dvar and of hbar*ens, summed exactly as the flow statistics' series (per
 * element the products jac_I * x_I added in node order from the first, the element sums by the pairwise
 * tree over the element positions; the host adds the ranks).  No series, no floating-point atomics.
 * Every value has the bits of the numpy mirror hnumo/covariance.py (HostEddyCov) on the synced states.
 * Nodes of ghost elements are never accumulated and read 0 everywhere.  DESIGN.md §6.1.7.
 *
 * hnumo_cov_begin: coriolis_df(npoin) or NULL: f = 0; zref(npoin,nlayers) or NULL: 0.  every = 0: only
 *   hnumo_cov_accumulate takes samples; every = k >= 1: the engine also takes one after every k-th
 *   successful hnumo_ti_rk_bcl (hnumo_group_ti_rk_bcl for grouped engines) since begin, once the step's
 *   abort / retry handling has finished, after the flow statistics' and the vorticity's sample and before
 *   the sample sets (a COV set sees the new sums) and the floats; a step that returns non-zero is not
 *   sampled.  A second call resets.  nlayers must be 2 or 3 and ngl 3, 4, 5, 6 or 8.  Independent of
 *   hnumo_stats_* and hnumo_vort_*: neither needs to be on.
 * hnumo_cov_accumulate: one sample of the state on the device, ordered after the step on the engine's
 *   stream, outside the captured step, nothing copied back: the step's launches, graph and bits are the
 *   same with covariances on or off.
 * hnumo_cov_sums / hnumo_cov_set_sums: out / in (14,npoin,nlayers) = S_h, S_u, S_v, S_uh, S_vh, S_uuh,
 *   S_uvh, S_vvh, S_d, S_dd, S_a, S_ua, S_va, S_qa in the index order of hnumo_layer_fields,
 *   n = 14*npoin*nlayers, and the sample count: a restarted run restores them and goes on.
 * hnumo_cov_fields: out(16,npoin,nlayers) = hbar, ubar, vbar, um, vm, Ruu, Ruv, Rvv, Fu, Fv, dbar, dvar,
 *   qm, Qu, Qv, ens; n = 16*npoin*nlayers.
 * hnumo_cov_integrals: out(3,nlayers), n = 3*nlayers.
 * hnumo_cov_end: frees the buffers; a no-op before hnumo_cov_begin.
 * All return 4, with a message in hnumo_last_error, before hnumo_cov_begin, for a wrong n or a negative
 * every; a sample returns 4 before any state was uploaded; hnumo_cov_fields and hnumo_cov_integrals
 * return 4 with no samples.                                                                       */
int hnumo_cov_begin(hnumo_engine *eng, const double *coriolis_df, const double *zref, int32_t every);
int hnumo_cov_accumulate(hnumo_engine *eng);
int hnumo_cov_sums(hnumo_engine *eng, double *out, int64_t n, int64_t *nsamples);
int hnumo_cov_set_sums(hnumo_engine *eng, const double *in, int64_t n, int64_t nsamples);
int hnumo_cov_fields(hnumo_engine *eng, double *out, int64_t n);
int hnumo_cov_integrals(hnumo_engine *eng, double *out, int64_t n);
int hnumo_cov_end(hnumo_engine *eng);

/* Energy budget on the device state (additive in ABI v10): the power the wind puts into the top layer, the
 * power the bottom drag removes, the interior viscous dissipation, and the kinetic and available potential
 * energy these change.  Wind work and drag are products of fields that decorrelate within a few steps, with
 * a wind that may change on the device every step (hnumo_wind_*), so they are formed where the state and
 * the wind live -- at the quadrature points, where the model applies its forcing -- and accumulated there.
 * Definitions (normative; IEEE double, no FMA, every sum left to right from its first product).  Owned
 * element e, nodes I = e*P + j*ngl + i, quad points Iq = e*Q + jq*nq + iq (nq = 2*ngl - 1, as creation
 * requires), w_I the nodal jac, wq_Iq the quad weight wjac, tau(1:2,Iq) the wind as it stands on the device
 * at the time of the sample: what hnumo_wind_get returns; after a scheduled step the row the step used.
 * At the nodes, per layer k:
 *   dp = q(1,I,k);  u = q(2,I,k)/dp;  v = q(3,I,k)/dp;  m = dp/gravity            (mass per area)
 *   ke_k  = (0.5*(u*u + v*v))*m
 *   z_k   = elevation of layer k's top interface as hnumo_layer_fields forms it (row 5)
 *   d_k   = z_k - zref(I,k)                                   (zref given at begin; NULL: 0.0)
 *   c_1   = 0.5*(gravity*(1.0/alpha_1));  c_k = 0.5*(gravity*(1.0/alpha_k - 1.0/alpha_(k-1)))  (k >= 2)
 *   ape_k = c_k*(d_k*d_k)
 *   u_x,u_y,v_x,v_y = the element's own gradient, the statements of hnumo_vort, unchanged
 *   eps_k = (visc_mlswe*((u_x*u_x + u_y*u_y) + (v_x*v_x + v_y*v_y)))*m
 * At the quad points, node->quad interpolation of a nodal field a(i,j) is done in two passes in this order:
 *   t(iq,n)  = psiq(1,iq)*a(1,n);  for m = 2..ngl: t = t + psiq(m,iq)*a(m,n)
 *   A(iq,jq) = psiq(1,jq)*t(iq,1); for n = 2..ngl: A = A + psiq(n,jq)*t(iq,n)
 * It is applied to u_1, v_1 (top layer) and u_L, v_L, dp_L (bottom layer; for nlayers = 1 the same layer),
 * giving U1, V1, UL, VL, DPL.  Then
 *   W = tau(1,Iq)*U1 + tau(2,Iq)*V1
 *   botfr == 0:  D = +0.0                                         (nothing interpolated for it)
 *   botfr == 1:  spd = (cd_mlswe/gravity)*DPL
 *   botfr == 2:  spd = (cd_mlswe/alpha_L)*sqrt(UL*UL + VL*VL)
 *                tb_u = spd*UL;  tb_v = spd*VL;  D = tb_u*UL + tb_v*VL
 * Units follow from mod_rhs_btp.F90:171, d(u dp)/dt = gravity*(tau - tb) + ...: tau and tb are stresses,
 * m = dp/g is mass per area, and W, D, eps are W/m^2.  Sign convention:
 * d(sum KE + sum APE)/dt ~ W - D - sum eps.
 * What the terms are and what they are not: the drag law is that of mod_rhs_btp.F90:157-168 evaluated on
 * the layer state q, not on the sub-cycle's (qb, qprime) split or on its time average; the wind is credited
 * to the top layer; eps is the interior estimate, without the LDG face terms; the KE<->APE conversion term
 * is not formed.  The budget therefore closes to discretisation error, not to bits.
 * One SAMPLE accumulates running sums (plain adds in sample order from +0.0; one lane owns a sum):
 * S_W += W and S_D += D per quad point, S_V += eps_k per node and layer.  With a series, one sample also
 * appends 3*nlayers + 2 integrals over the rank's owned elements: KE_1..L, APE_1..L, V_1..L, W, D -- nodal
 * rows the products w_I*x_I added in node order per element, quad rows wq_Iq*x_Iq in quad order, starting
 * from the first; the element sums combined by the position-defined pairwise tree of the flow statistics'
 * series; the host adds the ranks.  No floating-point atomics.  Ghost elements are never visited and read 0.
 * Every value has the bits of the numpy mirror hnumo/energy.py (HostEnergy).  DESIGN.md §6.1.8.
 *
 * hnumo_energy_begin: zref(npoin,nlayers) or NULL: 0.  every and series_capacity as hnumo_stats_begin's:
 *   every = 0: only hnumo_energy_sample takes samples; every = k >= 1: the engine also takes one after
 *   every k-th successful hnumo_ti_rk_bcl (hnumo_group_ti_rk_bcl for grouped engines) since begin, once
 *   the step's abort / retry handling has finished (a step redone after a persistent abort is sampled
 *   once), after the eddy covariances' sample and before the sample sets and the floats; a step that
 *   returns non-zero is not sampled.  series_capacity = 0: sums only.  A second call resets.  nlayers 1..3
 *   and every ngl the engine accepts.
 * hnumo_energy_sample: one sample now: plain launches on the engine's stream outside the captured step,
 *   nothing copied back; the step's launches, graph and bits are the same with the observer on or off.
 * hnumo_energy_series: out(3*nlayers+2, count), n >= (3*nlayers+2)*count; out = NULL returns the count;
 *   clear != 0 empties the series after the read.
 * hnumo_energy_sums / hnumo_energy_set_sums: quad2(2,npoin_q) = S_W, S_D, nq2 = 2*npoin_q;
 *   nodal(npoin,nlayers) = S_V, nn = npoin*nlayers; and the sample count: a restarted run restores them.
 * hnumo_energy_means: S_W/N, S_D/N and S_V/N, N = double(samples): the maps of mean wind power input, drag
 *   and dissipation.
 * hnumo_energy_end: frees the buffers; a no-op before hnumo_energy_begin.  hnumo_engine_destroy frees a
 *   begun observer.
 * All return 4, with the call and the value in hnumo_last_error: before hnumo_energy_begin, for a wrong n,
 * nq2 or nn, a negative every or capacity; a sample returns 4 when the series is full (nothing is
 * accumulated; the step itself is done) and before any state was uploaded; hnumo_energy_means with no
 * samples; hnumo_energy_series with no series.                                                     */
int hnumo_energy_begin(hnumo_engine *eng, const double *zref, int32_t every, int32_t series_capacity);
int hnumo_energy_sample(hnumo_engine *eng);
int hnumo_energy_series(hnumo_engine *eng, double *out, int64_t n, int64_t *count, int32_t clear);
int hnumo_energy_sums(hnumo_engine *eng, double *quad2, int64_t nq2, double *nodal, int64_t nn, int64_t *nsamples);
int hnumo_energy_set_sums(hnumo_engine *eng, const double *quad2, int64_t nq2, const double *nodal, int64_t nn,
                          int64_t nsamples);
int hnumo_energy_means(hnumo_engine *eng, double *quad2, int64_t nq2, double *nodal, int64_t nn);
int hnumo_energy_end(hnumo_engine *eng);

/* Region sets (additive in ABI v10): the integral series of PARTS of the rank's domain -- subpolar against
 * subtropical gyre, the western boundary strip against the interior, zonal strips whose per-layer
 * meridional transport, cumulated over the layers, is the overturning streamfunction in layer space --
 * formed where the state lives, by a segmented tree reduction: many regions at once, each with its own
 * position-defined tree, in a number of launches that does not grow with the number of regions.
 * Definitions (normative; the same text in csrc/region_plan.h, csrc/kernels_region.hip
 * and hnumo/regions.py).  A region set labels every owned element with a region r in 0..R; label 0: the
 * element is in no region.  Up to HNUMO_REGION_MAXSETS = 4 sets exist at once (overlapping partitions,
 * such as strips and basins, are separate sets).  The members of region r, in ascending local element
 * number, have local positions 0..n_r-1.  IEEE double, -ffp-contract=off: no FMA; IEEE division; every sum
 * left to right from its first product.  Per member element e, layer k, node I = e*P + j*ngl + i, w_I the
 * nodal jac:
 *   FLOW rows (HNUMO_REGION_FLOW, mask bit 0), the statements of hnumo_stats_*:
 *     dp = q(1); h = (alpha_k/gravity)*dp; u = q(2)/dp; v = q(3)/dp
 *     VOL_k = int h;  TU_k = int (u*h);  TV_k = int (v*h);  KE_k = int ((0.5*(u*u+v*v))*h)
 *   VORT rows (HNUMO_REGION_VORT, mask bit 1), the statements of hnumo_vort_*; f the caller's
 *   coriolis_df, 0 for NULL:
 *     Z_k = int ((0.5*(zeta*zeta))*h);  PZ_k = int ((0.5*(pv*pv))*h);  G_k = int zeta
 * `int` in two steps: per element the products w_I*x_I added in node order from the first product; per
 * region the element sums combined by the flow statistics' pairwise tree over the LOCAL POSITIONS (entry i
 * of the next level is x[2i] + x[2i+1], or x[2i] alone where 2i+1 does not exist).  An empty region reads
 * +0.0 in every row.  No floating-point atomics.  Ghost elements are never members.
 * Entry: (V, R), V = 4*nlayers*[FLOW] + 3*nlayers*[VORT]; FLOW rows first, 4(k-1) + {0 VOL, 1 TU, 2 TV,
 * 3 KE}, then the VORT rows, 3(k-1) + {0 Z, 1 PZ, 2 G} (hnumo_vort_series' order).  A set whose only region
 * holds all owned elements has local position = element position: its KE_k, VOL_k are the bits of
 * hnumo_stats_series, its Z_k, PZ_k, G_k those of hnumo_vort_series.  Every value has the bits of the numpy
 * mirror hnumo/regions.py (HostRegions).
 * Out of scope: labels per node (strips finer than an element; sample sets cover lines); fluxes across
 * region boundaries (they need the step's own face fluxes); combining ranks (the host adds them, as for the
 * other series).
 *
 * hnumo_regions_create: region_of_elem(n), n = nelem_owned, labels 0..nregions; rows_mask as above;
 *   coriolis_df(npoin) or NULL (read with HNUMO_REGION_VORT only).  every = 0: only hnumo_regions_sample
 *   takes samples; every = k >= 1: the engine also takes one after every k-th successful hnumo_ti_rk_bcl
 *   (hnumo_group_ti_rk_bcl for grouped engines) since create, once the step's abort / retry handling has
 *   finished (a step redone after a persistent abort is sampled once), after the energy budget's sample and
 *   before the sample sets and the floats; a step that returns non-zero is not sampled.  series_capacity:
 *   samples the series can hold.  The regions' areas are formed here, once.  An engine that creates no set
 *   launches what it launched before.
 * hnumo_regions_sample: one sample now into the series: one launch over the set's member elements (cost
 *   follows the members, not the mesh) and ceil(log_1024 max_r n_r) >= 1 tree launches, whatever nregions
 *   is; plain launches on the engine's stream outside the captured step, nothing copied back; the step's
 *   launches, graph and bits are the same with or without region sets.
 * hnumo_regions_series: out(V, nregions, count), n >= V*nregions*count; out = NULL returns the count;
 *   clear != 0 empties the series after the read.
 * hnumo_regions_area: out(nregions), n = nregions: sum of w_I per region, by the same per-element order and
 *   the same tree with x = 1.0.
 * hnumo_regions_destroy: frees the set; hnumo_engine_destroy frees what is left.
 * All return 4, with the call and the value in hnumo_last_error: for an unknown id; hnumo_regions_create,
 * checked in this order, for id NULL, a negative every or capacity, unsupported nlayers or ngl (nlayers
 * 1..3; ngl 3, 4, 5, 6 or 8: what hnumo_vort_begin accepts), region_of_elem NULL, nregions < 1,
 * n != nelem_owned, a rows_mask that is empty or holds other bits, a label outside 0..nregions, a fifth set;
 * a sample before any state was uploaded, on a set with capacity 0, or when the series is full (nothing is
 * recorded; the step itself is done); hnumo_regions_series on a set with capacity 0 or with too small an
 * n; hnumo_regions_area with n != nregions.                                                         */
#define HNUMO_REGION_MAXSETS 4
#define HNUMO_REGION_FLOW 1
#define HNUMO_REGION_VORT 2
int hnumo_regions_create(hnumo_engine *eng, const int32_t *region_of_elem, int64_t n, int32_t nregions, int32_t rows_mask,
                         const double *coriolis_df, int32_t every, int32_t series_capacity, int32_t *id);
int hnumo_regions_sample(hnumo_engine *eng, int32_t id);
int hnumo_regions_series(hnumo_engine *eng, int32_t id, double *out, int64_t n, int64_t *count, int32_t clear);
int hnumo_regions_area(hnumo_engine *eng, int32_t id, double *out, int64_t n);
int hnumo_regions_destroy(hnumo_engine *eng, int32_t id);

/* Sample sets (additive in ABI v10): the state on the device, or the accumulated flow statistics,
 * evaluated at arbitrary points -- a regular output grid, a cross-section, a few stations -- by the
 * element's own Lagrange interpolant, where the post-processing scripts griddata the synced nodal
 * values (Examples/double_gyre/compute_ssh.m:58-70, compute_ke.m, plot_gyre.m, Examples/bump/
 * plot_bump*.m, Examples/lake/plot_lake_2D.m).  On demand, or after every k-th step into a series
 * kept on the device: a station series from every step without one hnumo_sync.  DESIGN.md §6.1.2.
 *
 * A set is M points, each a 1-based local element (0: not on this rank) and reference coordinates
 * (xi, eta) in [-1,1]^2, with the 1-D LGL nodes xgl(ngl) (mod_basis xgl).  Weights, once per set on
 * the host: Lx[i] = l_i(xi) by w = 1; for m = 0..ngl-1, m != i: w = w * ((xi - xgl[m]) / (xgl[i] -
 * xgl[m])) (each factor a quotient first, multiplied in the order of m); Ly[j] from eta likewise.
 * Nodal fields of the element, node I = e*P + j*ngl + i:
 *   HNUMO_SAMPLE_STATE  V = 5*nlayers + 4 values per point: rows 5(k-1)+1..5k = layer k's h, u, v,
 *                       dp, elevation exactly as hnumo_layer_fields forms them, then qb_df(1:4, I)
 *   HNUMO_SAMPLE_STATS  V = 5*nlayers: hbar, um, vm, mke, eke of hnumo_stats_fields per layer
 *   HNUMO_SAMPLE_VORT   V = 4*nlayers: zeta, delta, pv, ow of hnumo_vort_fields per layer, formed from
 *                       the set's own elements (f as hnumo_vort_begin took it)
 *   HNUMO_SAMPLE_COV    V = 16*nlayers: the 16 fields of hnumo_cov_fields per layer, interpolated as
 *                       the STATS source is
 * Value: val = sum_j Ly[j] * r_j with r_j = sum_i Lx[i] * F(e, j*ngl + i), both sums left to right
 * from their first product (no FMA).  Points with elem = 0 read 0.0 in every row.  At xi = xgl[a],
 * eta = xgl[b] the weights are exactly 0 and 1: the sample is the nodal value.  Every value has the
 * bits of the numpy mirror hnumo/sample.py (HostSampler) on the synced state.
 *
 * hnumo_sample_create: locates xy(2,M) in the rank's OWNED elements from coord(ldc,npoin) (ldc = 2
 *   or 3, as hnumo_diag_geometry takes it).  Elements are straight-sided bilinear quadrilaterals
 *   (every node the bilinear map of the four corner nodes at (xgl(i), xgl(j)) to within 64 eps
 *   max|coord|: a curved element is an error).  The map is inverted with Newton; an element accepts
 *   a point when max(|xi|, |eta|) <= 1 + tol_e, tol_e = 64 eps max|coord| / (half the element's
 *   shortest edge); the lowest accepting element wins and (xi, eta) are clamped to [-1,1].  A point
 *   no element accepts (outside the rank's owned elements, or not finite) gets elem = 0.
 * hnumo_sample_create_ref: takes elem(M) in 0..nelem_owned and xi_eta(2,M) in [-1,1] as given.
 *   Both return the set's id (0..7: up to 8 sets per engine; hnumo_engine_destroy frees them).
 * hnumo_sample_plan: the set's elem(M) and xi_eta(2,M) (either may be NULL); M must be the set's.
 * hnumo_sample: samples now and copies out(V,M), n = V*M.
 * hnumo_sample_series_begin: (re)allocates the set's series of `capacity` samples on the device and
 *   empties it (capacity = 0: no series).  every = 0: only hnumo_sample_record appends; every =
 *   k >= 1: the engine also appends after every k-th successful hnumo_ti_rk_bcl (hnumo_group_ti_rk_bcl
 *   for grouped engines) since begin, once the step's abort / retry handling has finished and after
 *   the flow statistics' own sample of that step (a STATS set sees the new sums).  If the series is
 *   full then, the step call returns 4 (the step is done).
 * hnumo_sample_record: appends one sample to the series on the device; nothing is copied back.
 * hnumo_sample_series: out(V,M,count); n = the doubles out can hold, at least V*M*count; out = NULL
 *   (n = 0) only returns count.  clear = 1 empties the series after the copy.
 * hnumo_sample_destroy: frees the set; its id is given out again.
 * All launches are plain launches on the engine stream outside the captured step: the step's
 * launches, graph and bits are the same with or without sets.  All return 4, with a message in
 * hnumo_last_error, for an unknown id, a wrong n or M, negative arguments, invalid points or
 * geometry, a ninth set; a sample returns 4 before any state was uploaded, when the series is full
 * or absent, for a STATS set before hnumo_stats_begin or with no statistics samples, and for a VORT
 * set before hnumo_vort_begin or after hnumo_vort_end (the set needs f: creating it is refused too);
 * for a COV set before hnumo_cov_begin (creating it is refused too) or with no covariance samples. */
#define HNUMO_SAMPLE_STATE 0
#define HNUMO_SAMPLE_STATS 1
#define HNUMO_SAMPLE_VORT 2
#define HNUMO_SAMPLE_COV 3
int hnumo_sample_create(hnumo_engine *eng, const double *coord, int32_t ldc, const double *xgl, const double *xy,
                        int64_t M, int32_t source, int32_t *id);
int hnumo_sample_create_ref(hnumo_engine *eng, const double *xgl, const int32_t *elem, const double *xi_eta, int64_t M,
                            int32_t source, int32_t *id);
int hnumo_sample_plan(hnumo_engine *eng, int32_t id, int32_t *elem, double *xi_eta, int64_t M);
int hnumo_sample(hnumo_engine *eng, int32_t id, double *out, int64_t n);
int hnumo_sample_series_begin(hnumo_engine *eng, int32_t id, int32_t every, int32_t capacity);
int hnumo_sample_record(hnumo_engine *eng, int32_t id);
int hnumo_sample_series(hnumo_engine *eng, int32_t id, double *out, int64_t n, int64_t *count, int32_t clear);
int hnumo_sample_destroy(hnumo_engine *eng, int32_t id);

/* Float sets (additive in ABI v10): Lagrangian floats or drifters that live in a layer and move with
 * its velocity, advanced on the device after every step from the resident q_df -- a trajectory needs
 * the velocity at the float's own position at every step, which the mlswe#### snapshots cannot give
 * and a host pass pays one hnumo_sync per step for.  DESIGN.md §6.1.3.
 *
 * A set is M floats.  A float carries a position (x, y), a layer k (1-based, fixed for life), a stored
 * velocity w = (wx, wy), a cached location (elem, xi, eta) and a status: HNUMO_FLOAT_ACTIVE,
 * HNUMO_FLOAT_LEFT (it reached a processor face or a ghost element; also "not on this rank at
 * creation"), HNUMO_FLOAT_LOST.  All arithmetic is IEEE double without FMA; every value has the bits
 * of the numpy mirror hnumo/floats.py (HostFloats) on the synced states.
 *   vel(e, xi, eta): rows 5(k-1)+2, 5(k-1)+3 (u, v of layer k) of a hnumo_sample_create_ref set at
 *     (e, xi, eta): nodal q(2,I,k)/q(1,I,k), q(3,I,k)/q(1,I,k) under the element's interpolant.
 *   locate(p, e): (1) invert e's bilinear map at p (Newton from the element centre, at most 32
 *     iterations, the loop of hnumo_sample_create; no finite solution: LOST); (2) max(|xi|, |eta|) <=
 *     1 + tol_e (hnumo_sample_create's): clamp to [-1,1], accept; (3) else the side with the larger
 *     excess (|xi| - 1 against |eta| - 1, a tie goes to xi, the sign selects the face): an owned
 *     neighbour -> continue there at (1); a physical boundary (face(8) < 0) -> that coordinate = +-1
 *     exactly and p = e's map at the new (xi, eta) -- the float slides along the wall --, again (1)
 *     in e; a processor face (face(8) = 0) or a ghost neighbour -> LEFT; (4) a fifth pass through
 *     (3) -> LOST.
 *   advance by dt (Heun with the field of the new time level; w is from the previous one):
 *     if fresh: w = vel(elem, xi, eta), fresh = 0          (first advance after create / set)
 *     p* = (x + dt*wx, y + dt*wy);  (e*, xi*, eta*, p*) = locate(p*, elem);  u* = vel(e*, xi*, eta*)
 *     p1 = (x + (0.5*dt)*(wx + u*x), y + (0.5*dt)*(wy + u*y));  (e1, xi1, eta1, p1) = locate(p1, e*)
 *     w = vel(e1, xi1, eta1);  (x, y) = p1;  (elem, xi, eta) = (e1, xi1, eta1)
 *     A location that ends LEFT or LOST stops the advance: (x, y) = that location's target, elem = 0,
 *     w = 0; a non-finite velocity gives LOST likewise, at the target located last.  Inactive floats
 *     are never touched again.  On a processor-face partition a set that migrates (below) hands a
 *     float that reaches a processor face to the rank across it, inside the engine.
 *
 * Migration (hnumo_floats_migrate; processor-face engines, opt-in; a set that does not opt in is as above).
 *   Flight record.  When locate reaches (3) at a processor face (face(8) = 0) in a migrating set, the
 *     float is in flight instead of LEFT.  Its record carries: gid, its 0-based input index (every rank
 *     creates the set from the same xy(2,M), layer(M)); layer; the position (x, y) and velocity (wx, wy)
 *     it had at the start of this advance (after the fresh evaluation); dt; stage (0 while locating p*,
 *     1 while locating p1); the current target (px, py), as walls may have moved it; hops, the passes
 *     through (3) so far in this location, counting the one that reached the face; the destination:
 *     the neighbour index k in this rank's nbh_proc and the position pos of the face inside that
 *     neighbour's segment of nbh_send_recv (both ranks agree on that order: the halo descriptor's
 *     contract).
 *   Arrival.  The receiver's face at (its neighbour index for the sender, pos) gives the local element
 *     face(7).  locate continues there at (1) with the carried target and hop count; the advance goes
 *     on from the carried stage with the statements of advance -- stage 0: u* = vel, p1, a second
 *     location starting with hops = 0, w = vel; stage 1: w = vel.  The result goes into the receiver's
 *     own slot gid, which is LEFT there by construction.
 *   Sender's slot.  LEFT exactly as without migration: (x, y) = the target, elem = 0, w = 0.
 *   Further crossings.  A continuation may reach another processor face: another flight.  Every flight
 *     uses up at least one hop and a location allows four, so an advance settles in at most 8 rounds
 *     of arrivals; the round loop has that bound, and a float still in flight after round 8 is LOST
 *     where it left (this cannot happen).
 *   Tolerance.  tol_e depends on max|coord|, which a rank takes over its own nodes.  coord_scale > 0
 *     replaces it in tol_e for every later location of the set, so that all ranks and the single-rank
 *     run accept on the same threshold; 0 keeps the rank's own.  Seeds are not re-located.
 *   Seeds on shared edges.  A seed on an edge two ranks share is ACTIVE on both at creation; in a
 *     migrating set a float may be ACTIVE on one rank only.  hnumo_group_floats_migrate keeps it on the
 *     lowest rank that holds it and makes it LEFT (elem 0, w 0) on the others; hnumo_floats_release does
 *     the same for a host that transports the records itself.
 *   Per record at most one rank has elem > 0 for a float; that rank's record is the single-rank float's,
 *   bit for bit, through any number of crossings (with one coord_scale everywhere).
 *
 * hnumo_floats_migrate: on = 1 / 0, coord_scale as above.  4 on an engine without a processor-face halo
 *   (a single rank, a ghost-layer partition, the self-neighbour emulation), for a negative or non-finite
 *   scale, for an unknown id.  hnumo_floats_set on a migrating set re-seeds this rank alone.
 * hnumo_group_floats_migrate: the same on every engine of a local group, plus the shared-edge rule.
 * hnumo_group_floats_advance: every engine's advance of the set by dt, then rounds (at most 8, until no
 *   float is in flight): synchronise every engine's stream, read back the outbox counts, run the
 *   arrivals of every non-empty outbox on its receivers, flip the outboxes' parity.  The records that
 *   fell due are taken on every engine after the last round.  hnumo_group_ti_rk_bcl runs the same
 *   phase with params.dt for every migrating set with every = 1, after all engines' other observers:
 *   floats are still last, a refused recording still lets everything else run, and the first non-zero
 *   code is returned.
 * For a host that carries the records itself (one engine per process, MPI or RCCL between the GPUs;
 * transport of flight records over RCCL inside the engine is out of scope, these calls are its
 * interface): on such an engine an advance of a migrating set, explicit or after a step, defers the
 * record that falls due to hnumo_floats_settle.
 *   hnumo_floats_outbox: the flight records of the current outbox into d(cap,7) = x, y, wx, wy, dt, px,
 *     py and i(cap,6) = gid, layer, stage, hops, dest, pos, sorted by gid; dest is the destination's
 *     0-based rank (nbh_proc(k) - 1); *count of them.  The outbox is then empty: flights of later
 *     arrivals collect in it.  cap < count: 4, nothing taken.
 *   hnumo_floats_deliver: runs the arrivals of the n records that rank src_rank sent (those whose dest
 *     is another rank are dropped).  4 for a rank that shares no face with this one and for a record
 *     whose gid, layer, stage, hops or pos no sender produces.
 *   hnumo_floats_release: floats idx(n) (0-based input positions) that are ACTIVE here become LEFT.
 *   hnumo_floats_settle: takes the record that the advance deferred (none: nothing happens).
 *
 * hnumo_floats_create: coord(ldc,npoin), xgl(ngl) as hnumo_sample_create takes them (the same element
 *   contract and initial location); xy(2,M), layer(M) in 1..nlayers.  Returns the set's id (0..7: up to
 *   8 sets per engine; hnumo_engine_destroy frees them).  The side neighbours come from the mesh
 *   descriptor's face / imapl / imapr (the set of local nodes a face lists for an element: any local
 *   face numbering, either orientation); a mesh they cannot be derived from is an error here.
 * hnumo_floats_get: x, y, u, v, elem, status (M each, any may be NULL) in input order; u, v = w.
 * hnumo_floats_plan: the floats' cached locations elem(M), xi_eta(2,M) (either may be NULL) in input
 *   order: what a hnumo_sample_create_ref set takes.
 * hnumo_floats_set: re-seeds and relocates the set's M floats; fresh = 1.
 * hnumo_floats_advance: one advance by dt on the state on the device now.
 * hnumo_floats_begin: every = 1: the engine advances the set by params.dt after each successful
 *   hnumo_ti_rk_bcl (hnumo_group_ti_rk_bcl), once the step's abort / retry handling has finished and
 *   after the statistics' and the sample sets' own work; every = 0: only hnumo_floats_advance does;
 *   any other value is an error (a float cannot skip steps).  (Re)allocates the series of `capacity`
 *   records and empties it; a record is appended after every record_every-th advance since begin,
 *   explicit ones included (0: only hnumo_floats_record appends).  If the series is full then, the
 *   call returns 4 (the step and the advance are done).
 * hnumo_floats_record: appends one record to the series on the device; nothing is copied back.
 * hnumo_floats_series: out(5,M,count) = x, y, u, v, elem (as a double; 0: not on this rank) per record,
 *   in input order; n = the doubles out can hold; out = NULL (n = 0) only returns count; clear = 1
 *   empties the series after the copy.
 * hnumo_floats_destroy: frees the set; its id is given out again.
 *
 * Sensors (additive in ABI v10): what a float measures on the way.  A set has a sensor mask,
 * HNUMO_FLOAT_SENSE_STATE (1) + HNUMO_FLOAT_SENSE_VORT (2); the rows are those of the float's own layer k:
 *   STATE  S1 = 5 rows h, u, v, dp, elevation: rows 5(k-1)+1..5k of a HNUMO_SAMPLE_STATE set;
 *   VORT   S2 = 4 rows zeta, delta, pv, ow: rows 4(k-1)+1..4k of a HNUMO_SAMPLE_VORT set, f as
 *          hnumo_vort_begin took it.
 *   STATE rows come first; S is the sum over the set bits.
 * The value of a row for a float with elem > 0 is exactly what a hnumo_sample_create_ref set reads in that row
 * at the float's cached (elem, xi, eta), on the state on the device now: the nodal fields are formed by the
 * same statements; the weights are w = w*((xi - xgl[m])/(xgl[i] - xgl[m])) in the order of m (the statement
 * vel uses; hnumo/sample.py's lagrange_weights is its mirror); val = sum_j Ly[j]*(sum_i Lx[i]*F), left to
 * right from the first product, no FMA.  A float with elem = 0 (LEFT, LOST, not on this rank) reads 0.0 in
 * every row.  The STATE rows u, v therefore equal the record's own u, v bit for bit after an advance.
 * hnumo_floats_sensors: sets the mask (0: no sensors).  4 for an unknown id, an unknown bit, the VORT bit
 *   before hnumo_vort_begin (the rule of a HNUMO_SAMPLE_VORT set), and when the set's series has capacity > 0
 *   and the mask would change its width: sensors first, then hnumo_floats_begin; to change the mask later,
 *   begin with capacity 0 first.
 * hnumo_floats_begin allocates the series at 5 + S rows; hnumo_floats_record and the record that falls due
 *   after an advance append x, y, u, v, elem and the S sensor rows of the state on the device at that moment
 *   (after a step: the new time level at the new position; in a group: after the last round of arrivals, on
 *   the rank that holds the float); hnumo_floats_series returns out(5+S,M,count).
 * hnumo_floats_sense: the sensors now, out(S,M) in input order, n = S*M.  4 for S = 0, before any state was
 *   uploaded, and when the mask holds VORT and hnumo_vort_end has been called.  A record meets the same
 *   refusals; one that falls due is then reported like a full series: the step and the advance are done, the
 *   other observers still run and the first non-zero code is returned.
 * hnumo_floats_sense_info: S and K, the element slots the sensor kernel's arena holds for this set (0 without
 *   sensors); either pointer may be NULL.
 * A set whose mask is 0 is the set described above: the same launches, series width, bytes and messages.
 *
 * All launches are plain launches on the engine stream outside the captured step: the step's
 * launches, graph and bits are the same with or without sets.  All return 4, with a message in
 * hnumo_last_error, for an unknown id, a wrong M or n, invalid arguments or geometry, a ninth set;
 * an advance returns 4 before any state was uploaded and for a dt that is not finite.           */
#define HNUMO_FLOAT_ACTIVE 0
#define HNUMO_FLOAT_LEFT 1
#define HNUMO_FLOAT_LOST 2
int hnumo_floats_create(hnumo_engine *eng, const double *coord, int32_t ldc, const double *xgl, const double *xy,
                        const int32_t *layer, int64_t M, int32_t *id);
int hnumo_floats_get(hnumo_engine *eng, int32_t id, double *x, double *y, double *u, double *v, int32_t *elem,
                     int32_t *status, int64_t M);
int hnumo_floats_plan(hnumo_engine *eng, int32_t id, int32_t *elem, double *xi_eta, int64_t M);
int hnumo_floats_set(hnumo_engine *eng, int32_t id, const double *xy, const int32_t *layer, int64_t M);
int hnumo_floats_advance(hnumo_engine *eng, int32_t id, double dt);
int hnumo_floats_begin(hnumo_engine *eng, int32_t id, int32_t every, int32_t record_every, int32_t capacity);
int hnumo_floats_record(hnumo_engine *eng, int32_t id);
int hnumo_floats_series(hnumo_engine *eng, int32_t id, double *out, int64_t n, int64_t *count, int32_t clear);
int hnumo_floats_destroy(hnumo_engine *eng, int32_t id);
int hnumo_floats_migrate(hnumo_engine *eng, int32_t id, int32_t on, double coord_scale);
int hnumo_floats_release(hnumo_engine *eng, int32_t id, const int32_t *idx, int64_t n);
int hnumo_floats_outbox(hnumo_engine *eng, int32_t id, double *d, int32_t *i, int64_t cap, int64_t *count);
int hnumo_floats_deliver(hnumo_engine *eng, int32_t id, int32_t src_rank, const double *d, const int32_t *i, int64_t cap,
                         int64_t n);
int hnumo_floats_settle(hnumo_engine *eng, int32_t id);
#define HNUMO_FLOAT_SENSE_STATE 1
#define HNUMO_FLOAT_SENSE_VORT 2
int hnumo_floats_sensors(hnumo_engine *eng, int32_t id, int32_t mask);
int hnumo_floats_sense(hnumo_engine *eng, int32_t id, double *out, int64_t n);
int hnumo_floats_sense_info(hnumo_engine *eng, int32_t id, int32_t *nrows, int32_t *K);

/* Time-dependent wind stress (additive in ABI v10; no reference counterpart: the reference sets
 * tau_wind once, initial_conditions.F90:190, and reads it as plain data).  A few wind patterns are
 * uploaded once and a linear combination of them is formed on the device, so a wind that is ramped
 * up or follows a seasonal cycle needs neither a new engine nor a copy per step.  Arithmetic
 * (normative; IEEE double, no FMA), per component and quad point, for patterns T_m(2,npoin_q),
 * m = 0..M-1 with 1 <= M <= HNUMO_WIND_MAXM, over every local element (the ghost elements of a
 * ghost-layer partition included), and coefficients c_0..c_{M-1}:
 *     tau = c_0*T_0;  for m = 1..M-1: tau = tau + c_m*T_m        (left to right, product first)
 *     s = 0.0;  N_btp times: s = s + tau;  tau_wind_ave = s / double(N_btp)
 * An engine whose wind was set to tau is, bit for bit, an engine created with tau.
 *   hnumo_wind_begin     patterns(2,npoin_q,M), n = 2*npoin_q*M; keeps a copy of the create-time wind.
 *                        The wind is unchanged until a set or a scheduled step.  Again: replaces
 *                        the patterns and clears the schedule.
 *   hnumo_wind_set       blends now: for every later step, parity hook and hnumo_bench_steps.
 *   hnumo_wind_schedule  coef(M,nrows) is copied to the device once.  With k the number of successful
 *                        hnumo_ti_rk_bcl / hnumo_group_ti_rk_bcl calls since this call, step k uses row
 *                        r = first + k, applied before the step's launches: HNUMO_WIND_HOLD keeps the
 *                        last row beyond the table (and launches nothing more), HNUMO_WIND_REPEAT takes
 *                        r mod nrows.  nrows = 0 clears the schedule.  A step that returns non-zero
 *                        leaves k where it was; a step the engine redoes after a persistent launch
 *                        gave up consumes one row.  The parity hooks, hnumo_bench_steps and
 *                        hnumo_step_breakdown use the wind in place and never advance k.  In a local
 *                        group every engine follows its own schedule.
 *   hnumo_wind_get       the current tau_wind (n = 2*npoin_q) and the row the next step will use
 *                        (-1: no schedule).
 *   hnumo_wind_end       restores the create-time wind, bit for bit, and frees everything
 *                        (hnumo_engine_destroy frees a begun wind too).
 * Code 4, with the call and the value in the message: M outside 1..HNUMO_WIND_MAXM or different from
 * begin's, a NULL pointer, a wrong n, set / schedule / get / end before begin, nrows < 0, first < 0,
 * an unknown mode.                                                                         */
#define HNUMO_WIND_MAXM 4
#define HNUMO_WIND_HOLD 0
#define HNUMO_WIND_REPEAT 1
int hnumo_wind_begin(hnumo_engine *eng, const double *patterns, int64_t n, int32_t M);
int hnumo_wind_set(hnumo_engine *eng, const double *coef, int32_t M);
int hnumo_wind_schedule(hnumo_engine *eng, const double *coef, int32_t M, int32_t nrows, int32_t first, int32_t mode);
int hnumo_wind_get(hnumo_engine *eng, double *tau, int64_t n, int32_t *next_row);
int hnumo_wind_end(hnumo_engine *eng);

/* Summation order of the barotropic stage (no reference counterpart: the reference has
 * one order).  HNUMO_SUM_REFERENCE (the default) evaluates the volume integral and the
 * nodal -> quad interpolation as the reference's dense psih/dpsidx sums in its order:
 * results bit-identical to the reference Fortran.  HNUMO_SUM_FACTORED uses tensor-product
 * sum factorisation (~7x fewer flops, ~1.4x faster stage).  It is exact up to rounding,
 * but the momentum RHS is a difference of terms ~1e7 times larger, so reordering moves
 * it by up to ~1e-6 relative and the state by ~1e-7 relative after a few steps: outside
 * the 1e-10 parity bar, hence opt-in.  Environment override at create:
 * HNUMO_SUMMATION=reference|factored (any other value: create fails with code 4).
 * hnumo_get_summation returns the mode.                                               */
#define HNUMO_SUM_REFERENCE 0
#define HNUMO_SUM_FACTORED 1
int hnumo_set_summation(hnumo_engine *eng, int mode);
int hnumo_get_summation(hnumo_engine *eng);

/* How the barotropic stages run: 1 = one persistent launch per sub-cycle
 * (btp_subcycle_kernel; single-rank engines whose elements all fit on the device at once,
 * unless HNUMO_PERSISTENT=0 at create), 0 = one launch per stage (btp_stage_kernel).
 * Both give the same bits.                                                            */
int hnumo_stage_path(hnumo_engine *eng);

/* Which variants of the device code this engine launches (additive in ABI v10; no device work).
 * out[0]: the LDS arena of the per-stage barotropic kernel -- 5 or 4: a LEAN arena of large meshes
 * (the default from 2,048 owned elements on: 5), 0: the arena of small meshes; always 0 unless
 * N = 4 and the summation is HNUMO_SUM_REFERENCE, where the kernel has one arena.  out[1]: 1 when
 * the layer mass / consistency element kernels are the large-mesh ones (one quad row per term
 * chunk; the default from 2,048 owned elements on), else 0.  All variants give the same bits. */
int hnumo_kernel_variants(hnumo_engine *eng, int32_t out[2]);

/* Residency of the persistent sub-cycle launch (ABI v6).  The launch is used only when
 * every element's workgroup can be resident at once: the occupancy estimate says so, a
 * stage-less trial launch at create finds all workgroups resident, and every launch
 * checks again (a rendezvous that gives up after 20 ms instead of waiting on a workgroup
 * that cannot start).  A launch that gives up does no work; the engine then suspends the
 * persistent path, repeats the affected steps on per-stage launches (same bits) and, after
 * a back-off of 1, 2, 4 ... 1024 runs, re-probes with a stage-less trial launch: resident
 * again -> persistent again (ABI v7).
 * out[8] = {stage path (as hnumo_stage_path), estimated workgroups per CU (reference /
 * factored summation), CU count, trial launch outcome (reference / factored: 1 resident,
 * 0 not, -1 not run), runs that fell back, LDS bytes per workgroup}.                   */
int hnumo_persistent_info(hnumo_engine *eng, int32_t *out8);

/* The persistent path over the engine's life (ABI v7): out[4] = {launches that gave up,
 * trial re-probes, re-probes that found the grid resident again, runs before the next
 * re-probe (-1: the path is not suspended)}.                                          */
int hnumo_persistent_stats(hnumo_engine *eng, int32_t *out4);

/* Test hook (ABI v7): the k-th persistent sub-cycle launch from now (0 = the next) gives
 * up exactly as a launch whose workgroups are not all resident does.                  */
int hnumo_debug_force_abort(hnumo_engine *eng, int k);

/* Emulation hook (ABI v10; self-neighbour engines only: a one-rank communicator whose
 * processor faces are listed under the rank itself, bench.py --emulate): on = 1 freezes the
 * halo -- every exchange site sends the message it sent first, again and again (same sizes,
 * offsets and transport calls), so each processor face keeps the at-rest neighbour of an at-rest
 * case instead of its own traces.  Set before the first step.  Returns 4 on any
 * other engine.                                                                          */
int hnumo_debug_frozen_halo(hnumo_engine *eng, int on);

/* RCCL unique id (128 bytes) for hnumo_halo_desc.comm_id: generated by one rank and
 * broadcast by the host (MPI / torch.distributed) before hnumo_engine_create.        */
int hnumo_rccl_unique_id(unsigned char *out128);

/* Join the n engines of one process (one per rank 0..n-1 of the same partition, on the
 * same device) into a local exchange group: they share one stream and exchange ghost
 * data by device copies.  hnumo_group_ti_rk_bcl then advances all of them one step
 * (one host thread per engine).  For tests of the multi-rank path on one GPU.        */
int hnumo_local_group(hnumo_engine **engines, int n);
int hnumo_group_ti_rk_bcl(hnumo_engine **engines, int n, double **q_df, double **qb_df, double **qprime_df);
/* migrating float sets of a local group (see the float sets above); engines: the group's, in rank order */
int hnumo_group_floats_migrate(hnumo_engine **engines, int n, int32_t id, int32_t on, double coord_scale);
int hnumo_group_floats_advance(hnumo_engine **engines, int n, int32_t id, double dt);

/* Timing hook for the benchmark: run `nsteps` resident baroclinic steps and return
 * device-side event timings (ms) of the whole span and of the dominant kernel.       */
int hnumo_bench_steps(hnumo_engine *eng, int nsteps, double *ms_total,
                      double *ms_kernel_avg, int64_t *kernel_launches);

/* Average duration (ms) of the fused barotropic stage kernel, from HIP events recorded
 * on the engine stream around `nsubcycles` direct (non-graph) corrector sub-cycles of the
 * current device state (qb is not modified).                                          */
int hnumo_time_stage_kernel(hnumo_engine *eng, int nsubcycles, double *ms_kernel_avg);

/* Diagnostics: per-element phase clocks of the last stage launch, [nelem][32] uint64
 * (diagnostics builds, -DHNUMO_DIAG=1, with HNUMO_STAGE_PROF=1 in the environment).   */
int hnumo_debug_stage_profile(hnumo_engine *eng, uint64_t *out, int64_t n);

/* Per-kernel breakdown of a step (ABI v8; single-rank engines, resident uploaded state):
 * `nsteps` direct steps of the device state with an event after every launch on the
 * engine stream.  On return `*count` kernel families (in launch order) with their names
 * '\n'-joined in `names` (names_len bytes incl. the terminator) and their microseconds
 * per step in us_per_step[0..count).  The state advances by nsteps steps.               */
int hnumo_step_breakdown(hnumo_engine *eng, int nsteps, char *names, int64_t names_len,
                         double *us_per_step, int max_kernels, int *count);

/* Environment settings the engine read at create (ABI v9), ';'-joined "NAME=value" (with
 * " (ignored: HNUMO_EXPERIMENTS!=1)" appended where not honoured); "" when none.  Public
 * settings: HNUMO_PERSISTENT=0, HNUMO_GRAPH=0|1 (launch schedule, same bits) and
 * HNUMO_SUMMATION.  Every other HNUMO_* knob is an A/B experiment switch honoured only
 * with HNUMO_EXPERIMENTS=1.  Returns 4 if `len` bytes (incl. the terminator) were too few
 * (the text is cut).                                                                   */
int hnumo_overrides(const hnumo_engine *eng, char *out, int64_t len);

/* Stream-copy bandwidth of `device` (ABI v8): 16-byte copy kernels between two buffers of
 * `bytes` each -- grid-stride with default and with non-temporal loads/stores, and a one-pass
 * non-temporal form -- each run `reps` times back to back between two events after one
 * untimed launch; out2 = {GB/s of the fastest variant (bytes read + written), its index 0..2}.
 * The measured denominator of the roofline.                                               */
int hnumo_stream_copy_bw(int device, int64_t bytes, int reps, double *out2);

#ifdef __cplusplus
}
#endif
#endif /* HNUMO_ENGINE_H */
