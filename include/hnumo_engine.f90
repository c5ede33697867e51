! hnumo_engine.f90 -- Fortran ISO_C_BINDING interface to libhnumo_engine (include/hnumo_engine.h).
!
! The derived types mirror the C descriptor structs field for field (same order, bind(C)
! layout); every array field is a type(c_ptr) to the caller's Fortran array.  The engine
! copies everything it needs during hnumo_engine_create, so the descriptors only have to
! stay valid for that call.  State arrays are passed by reference as assumed-size arrays.
!
! Build: amdflang -c include/hnumo_engine.f90   (any Fortran 2008 compiler).
! Link:  -L<repo>/h-numo_amd -lhnumo_engine -Wl,-rpath,<repo>/h-numo_amd
module hnumo_engine_c
    use iso_c_binding, only: c_int, c_int32_t, c_int64_t, c_double, c_ptr, c_char, c_null_ptr, &
        c_null_char, c_f_pointer, c_loc
    implicit none
    private

    integer(c_int), parameter, public :: HNUMO_OK = 0, HNUMO_ERR_NEGATIVE_THICKNESS = 1, &
        HNUMO_ERR_NONFINITE = 2, HNUMO_ERR_DEVICE = 3, HNUMO_ERR_INVALID = 4
    integer(c_int32_t), parameter, public :: HNUMO_SHEAR_CORRECTOR_REFERENCE = 0, &
        HNUMO_SHEAR_CORRECTOR_PREDICTED = 1
    integer(c_int), parameter, public :: HNUMO_ABI_EXPECTED = 10   ! must equal hnumo_abi_version()
    integer(c_int), parameter, public :: HNUMO_SUM_REFERENCE = 0, HNUMO_SUM_FACTORED = 1

    ! = hnumo_mesh_desc (mod_grid, mod_face, mod_basis, mod_metrics; optional dense tables)
    type, bind(C), public :: hnumo_mesh_desc
        integer(c_int32_t) :: nelem = 0, npoin = 0, npoin_q = 0, nface = 0
        integer(c_int32_t) :: ngl = 0, nq = 0, nlayers = 0
        type(c_ptr) :: face = c_null_ptr                       ! (8,nface)
        type(c_ptr) :: imapl = c_null_ptr, imapr = c_null_ptr ! (3,ngl,nface) = imapl(:,:,1,:)
        type(c_ptr) :: normal_vector = c_null_ptr             ! (3,ngl,nface)
        type(c_ptr) :: normal_vector_q = c_null_ptr           ! (3,nq,nface)
        type(c_ptr) :: jac_face = c_null_ptr                  ! (ngl,nface)
        type(c_ptr) :: jac_faceq = c_null_ptr                 ! (nq,nface)
        type(c_ptr) :: massinv = c_null_ptr                   ! (npoin)
        type(c_ptr) :: psiq = c_null_ptr, dpsiq = c_null_ptr  ! (ngl,nq)
        type(c_ptr) :: psi = c_null_ptr, dpsi = c_null_ptr    ! (ngl,ngl)
        type(c_ptr) :: ksiq_x = c_null_ptr, ksiq_y = c_null_ptr, etaq_x = c_null_ptr, &
            etaq_y = c_null_ptr, jacq = c_null_ptr            ! (nq,nq,nelem)
        type(c_ptr) :: ksi_x = c_null_ptr, ksi_y = c_null_ptr, eta_x = c_null_ptr, &
            eta_y = c_null_ptr, jac = c_null_ptr              ! (ngl,ngl,nelem)
        type(c_ptr) :: psih = c_null_ptr, dpsidx = c_null_ptr, dpsidy = c_null_ptr, wjac = c_null_ptr
        type(c_ptr) :: indexq = c_null_ptr
        type(c_ptr) :: dpsidx_df = c_null_ptr, dpsidy_df = c_null_ptr, wjac_df = c_null_ptr
        type(c_ptr) :: index_df = c_null_ptr
        type(c_ptr) :: imapl_q = c_null_ptr, imapr_q = c_null_ptr ! (3,nq,nface), method_visc == 1
    end type hnumo_mesh_desc

    ! = hnumo_static_desc (mod_initial.F90:42-53)
    type, bind(C), public :: hnumo_static_desc
        type(c_ptr) :: pbprime = c_null_ptr, pbprime_df = c_null_ptr
        type(c_ptr) :: one_over_pbprime = c_null_ptr, one_over_pbprime_df = c_null_ptr
        type(c_ptr) :: pbprime_face = c_null_ptr, pbprime_df_face = c_null_ptr
        type(c_ptr) :: one_over_pbprime_edge = c_null_ptr
        type(c_ptr) :: coeff_pbpert_L = c_null_ptr, coeff_pbpert_R = c_null_ptr, coeff_pbub_LR = c_null_ptr
        type(c_ptr) :: coeff_mass_pbub_L = c_null_ptr, coeff_mass_pbub_R = c_null_ptr, &
            coeff_mass_pbpert_LR = c_null_ptr
        type(c_ptr) :: alpha = c_null_ptr
        type(c_ptr) :: tau_wind = c_null_ptr, coriolis_quad = c_null_ptr, grad_zbot_quad = c_null_ptr
        type(c_ptr) :: zbot_df = c_null_ptr, zbot_face = c_null_ptr
        type(c_ptr) :: fdt2_bcl = c_null_ptr, a_bcl = c_null_ptr, b_bcl = c_null_ptr
        type(c_ptr) :: ssprk_a = c_null_ptr, ssprk_beta = c_null_ptr
    end type hnumo_static_desc

    ! = hnumo_params (mod_input, mod_constants, mod_initial N_btp)
    type, bind(C), public :: hnumo_params
        real(c_double) :: dt = 0, dt_btp = 0
        real(c_double) :: visc_mlswe = 0, cd_mlswe = 0, ad_mlswe = 0, gravity = 0
        integer(c_int32_t) :: N_btp = 0, kstages = 0, method_visc = 0, botfr = 0
        real(c_double) :: max_shear_dz = 0
        integer(c_int32_t) :: shear_corrector = 0, reserved = 0
    end type hnumo_params

    ! = hnumo_halo_desc (mod_parallel)
    type, bind(C), public :: hnumo_halo_desc
        integer(c_int32_t) :: rank = 0, nranks = 1, num_nbh = 0
        type(c_ptr) :: nbh_proc = c_null_ptr, num_send_recv = c_null_ptr, nbh_send_recv = c_null_ptr
        type(c_ptr) :: comm_id = c_null_ptr
        integer(c_int32_t) :: nelem_owned = 0
        type(c_ptr) :: num_ghost_send = c_null_ptr, ghost_send = c_null_ptr
        type(c_ptr) :: num_ghost_recv = c_null_ptr, ghost_recv = c_null_ptr
    end type hnumo_halo_desc

    public :: hnumo_engine_create, hnumo_engine_destroy, hnumo_abi_version, hnumo_ti_rk_bcl, &
        hnumo_ti_barotropic_ssprk, hnumo_btp_bcl_coeffs, hnumo_create_rhs_btp, hnumo_get_field_c, &
        hnumo_set_resident, hnumo_sync, hnumo_last_error_c, hnumo_last_error, hnumo_get_field, &
        hnumo_set_summation, hnumo_get_summation, hnumo_stage_path, hnumo_persistent_info, hnumo_predict, &
        hnumo_kernel_variants, &
        hnumo_rccl_unique_id, hnumo_persistent_stats, hnumo_diag_geometry, hnumo_diagnostics, &
        hnumo_layer_fields, hnumo_stats_begin, hnumo_stats_accumulate, hnumo_stats_sums, &
        hnumo_stats_set_sums, hnumo_stats_fields, hnumo_stats_series, hnumo_stats_end, &
        hnumo_vort_begin, hnumo_vort_fields, hnumo_vort_record, hnumo_vort_series, hnumo_vort_end, &
        hnumo_cov_begin, hnumo_cov_accumulate, hnumo_cov_sums, hnumo_cov_set_sums, hnumo_cov_fields, &
        hnumo_cov_integrals, hnumo_cov_end, &
        hnumo_energy_begin, hnumo_energy_sample, hnumo_energy_series, hnumo_energy_sums, hnumo_energy_set_sums, &
        hnumo_energy_means, hnumo_energy_end, &
        hnumo_regions_create, hnumo_regions_sample, hnumo_regions_series, hnumo_regions_area, hnumo_regions_destroy, &
        hnumo_sample_create, hnumo_sample_create_ref, hnumo_sample_plan, hnumo_sample, &
        hnumo_sample_series_begin, hnumo_sample_record, hnumo_sample_series, hnumo_sample_destroy, &
        hnumo_floats_create, hnumo_floats_get, hnumo_floats_plan, hnumo_floats_set, hnumo_floats_advance, &
        hnumo_floats_begin, hnumo_floats_record, hnumo_floats_series, hnumo_floats_destroy, &
        hnumo_floats_migrate, hnumo_floats_release, hnumo_floats_outbox, hnumo_floats_deliver, hnumo_floats_settle, &
        hnumo_floats_sensors, hnumo_floats_sense, hnumo_floats_sense_info, &
        hnumo_wind_begin, hnumo_wind_set, hnumo_wind_schedule, hnumo_wind_get, hnumo_wind_end
    integer(c_int32_t), parameter, public :: HNUMO_DIAG_MASS = 1   ! hnumo_diagnostics flags
    integer(c_int32_t), parameter, public :: HNUMO_SAMPLE_STATE = 0, HNUMO_SAMPLE_STATS = 1, &
        HNUMO_SAMPLE_VORT = 2, HNUMO_SAMPLE_COV = 3   ! sample set sources
    integer(c_int32_t), parameter, public :: HNUMO_REGION_MAXSETS = 4, HNUMO_REGION_FLOW = 1, HNUMO_REGION_VORT = 2
    integer(c_int32_t), parameter, public :: HNUMO_WIND_MAXM = 4, HNUMO_WIND_HOLD = 0, HNUMO_WIND_REPEAT = 1
    integer(c_int32_t), parameter, public :: HNUMO_FLOAT_ACTIVE = 0, HNUMO_FLOAT_LEFT = 1, HNUMO_FLOAT_LOST = 2   ! float status
    integer(c_int32_t), parameter, public :: HNUMO_FLOAT_SENSE_STATE = 1, HNUMO_FLOAT_SENSE_VORT = 2   ! sensor mask bits

    interface
        integer(c_int) function hnumo_engine_create(mesh, statics, params, halo, device, eng) &
                bind(C, name='hnumo_engine_create')
            import :: c_int, c_ptr, hnumo_mesh_desc, hnumo_static_desc, hnumo_params
            type(hnumo_mesh_desc), intent(in) :: mesh
            type(hnumo_static_desc), intent(in) :: statics
            type(hnumo_params), intent(in) :: params
            type(c_ptr), value :: halo                    ! hnumo_halo_desc* or c_null_ptr
            integer(c_int), value :: device
            type(c_ptr), intent(out) :: eng
        end function hnumo_engine_create

        subroutine hnumo_engine_destroy(eng) bind(C, name='hnumo_engine_destroy')
            import :: c_ptr
            type(c_ptr), value :: eng
        end subroutine hnumo_engine_destroy

        integer(c_int) function hnumo_abi_version() bind(C, name='hnumo_abi_version')
            import :: c_int
        end function hnumo_abi_version

        ! 128-byte RCCL unique id for hnumo_halo_desc%comm_id (made on one rank, broadcast)
        integer(c_int) function hnumo_rccl_unique_id(out128) bind(C, name='hnumo_rccl_unique_id')
            import :: c_int, c_char
            character(kind=c_char), intent(out) :: out128(128)
        end function hnumo_rccl_unique_id

        type(c_ptr) function hnumo_last_error_c(eng) bind(C, name='hnumo_last_error')
            import :: c_ptr
            type(c_ptr), value :: eng
        end function hnumo_last_error_c

        ! = ti_rk_bcl(q_df, qb_df, qprime_df)  (ti_rk_bcl.F90:9-87)
        integer(c_int) function hnumo_ti_rk_bcl(eng, q_df, qb_df, qprime_df) bind(C, name='hnumo_ti_rk_bcl')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(inout) :: q_df(*), qb_df(*), qprime_df(*)
        end function hnumo_ti_rk_bcl

        ! = ti_barotropic_ssprk_mlswe(qb_df, qprime_df)  (mod_rk_mlswe.F90:19-151)
        integer(c_int) function hnumo_ti_barotropic_ssprk(eng, qb_df, qprime_df) &
                bind(C, name='hnumo_ti_barotropic_ssprk')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(inout) :: qb_df(*)
            real(c_double), intent(in) :: qprime_df(*)
        end function hnumo_ti_barotropic_ssprk

        ! = btp_bcl_coeffs_qdf after extract_qprime_df_face  (ti_rk_bcl.F90:43-50)
        integer(c_int) function hnumo_btp_bcl_coeffs(eng, qprime_df) bind(C, name='hnumo_btp_bcl_coeffs')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: qprime_df(*)
        end function hnumo_btp_bcl_coeffs

        ! = create_rhs_btp(rhs, qb_df, qprime_df)  (mod_rhs_btp.F90:28-59)
        integer(c_int) function hnumo_create_rhs_btp(eng, rhs, qb_df, qprime_df) bind(C, name='hnumo_create_rhs_btp')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: rhs(*)
            real(c_double), intent(in) :: qb_df(*), qprime_df(*)
        end function hnumo_create_rhs_btp

        integer(c_int) function hnumo_get_field_c(eng, name, out, n) bind(C, name='hnumo_get_field')
            import :: c_int, c_ptr, c_char, c_double, c_int64_t
            type(c_ptr), value :: eng
            character(kind=c_char), intent(in) :: name(*)
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
        end function hnumo_get_field_c

        integer(c_int) function hnumo_set_resident(eng, on) bind(C, name='hnumo_set_resident')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
            integer(c_int), value :: on
        end function hnumo_set_resident

        ! summation order of the barotropic stage: HNUMO_SUM_REFERENCE (default, bitwise) or
        ! HNUMO_SUM_FACTORED (sum-factorised, opt-in; see include/hnumo_engine.h)
        integer(c_int) function hnumo_set_summation(eng, mode) bind(C, name='hnumo_set_summation')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
            integer(c_int), value :: mode
        end function hnumo_set_summation

        integer(c_int) function hnumo_get_summation(eng) bind(C, name='hnumo_get_summation')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_get_summation

        ! 1: one persistent launch per barotropic sub-cycle, 0: one launch per stage
        integer(c_int) function hnumo_stage_path(eng) bind(C, name='hnumo_stage_path')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_stage_path

        ! the device code variants launched, out(2) = (stage kernel arena 0 | 4 | 5, large-mesh
        ! mass / consistency kernels 0 | 1): see hnumo_engine.h
        integer(c_int) function hnumo_kernel_variants(eng, out) bind(C, name='hnumo_kernel_variants')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), intent(out) :: out(2)
        end function hnumo_kernel_variants

        ! residency of the persistent launch, out(8): see hnumo_engine.h
        integer(c_int) function hnumo_persistent_info(eng, out) bind(C, name='hnumo_persistent_info')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), intent(out) :: out(8)
        end function hnumo_persistent_info

        ! the persistent path over the engine's life, out(4): see hnumo_engine.h (ABI v7)
        integer(c_int) function hnumo_persistent_stats(eng, out) bind(C, name='hnumo_persistent_stats')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), intent(out) :: out(4)
        end function hnumo_persistent_stats

        ! the prediction half of ti_rk_bcl (ti_rk_bcl.F90:43-57): out q_df2, qb_df, qprime_df2
        integer(c_int) function hnumo_predict(eng, q_df, qb_df, qprime_df) bind(C, name='hnumo_predict')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(inout) :: q_df(*), qb_df(*), qprime_df(*)
        end function hnumo_predict

        integer(c_int) function hnumo_sync(eng, q_df, qb_df, qprime_df) bind(C, name='hnumo_sync')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: q_df(*), qb_df(*), qprime_df(*)
        end function hnumo_sync

        ! Run diagnostics on the device state (see include/hnumo_engine.h).  Once per engine:
        ! coord(ldc,npoin) = mod_grid coord (ldc = size(coord,1), 2 or 3), wjac_df(npoin) =
        ! c_loc(wjac_df) of mod_initial, or c_null_ptr: the nodal jac of the mesh descriptor
        integer(c_int) function hnumo_diag_geometry(eng, coord, ldc, wjac_df) bind(C, name='hnumo_diag_geometry')
            import :: c_int, c_int32_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: coord(*)
            integer(c_int32_t), value :: ldc
            type(c_ptr), value :: wjac_df
        end function hnumo_diag_geometry

        ! = the numbers of print_diagnostics_mlswe (print_diagnostics.F90:14-190) without hnumo_sync:
        ! out(12 + 11*nlayers) = [cfl_b, cfl, min_dx, min_dy, qbmax(4), qbmin(4)], then per layer
        ! [mass, qmax(5), qmin(5)]; flags = HNUMO_DIAG_MASS includes the layer masses
        integer(c_int) function hnumo_diagnostics(eng, flags, out, n) bind(C, name='hnumo_diagnostics')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: flags
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
        end function hnumo_diagnostics

        ! = q(5,npoin,nlayers) of diagnostics.F90:24-45 from the device state; n = 5*npoin*nlayers
        integer(c_int) function hnumo_layer_fields(eng, out5, n) bind(C, name='hnumo_layer_fields')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: out5(*)
            integer(c_int64_t), value :: n
        end function hnumo_layer_fields

        ! Online flow statistics on the device state (see include/hnumo_engine.h): time means,
        ! MKE / EKE and the KE series of the double-gyre post-processing, without hnumo_sync.
        ! Begin before the time loop (every = k >= 1: the engine samples after every k-th successful
        ! hnumo_ti_rk_bcl itself, so the loop does not change), fetch after it.
        integer(c_int) function hnumo_stats_begin(eng, every, series_capacity) bind(C, name='hnumo_stats_begin')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: every, series_capacity
        end function hnumo_stats_begin

        integer(c_int) function hnumo_stats_accumulate(eng) bind(C, name='hnumo_stats_accumulate')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_stats_accumulate

        ! out(4,npoin,nlayers) = S_h, S_uh, S_vh, S_e; n = 4*npoin*nlayers
        integer(c_int) function hnumo_stats_sums(eng, out, n, nsamples) bind(C, name='hnumo_stats_sums')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
            integer(c_int64_t), intent(out) :: nsamples
        end function hnumo_stats_sums

        integer(c_int) function hnumo_stats_set_sums(eng, sums, n, nsamples) bind(C, name='hnumo_stats_set_sums')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: sums(*)
            integer(c_int64_t), value :: n, nsamples
        end function hnumo_stats_set_sums

        ! out(5,npoin,nlayers) = hbar, um, vm, mke, eke; n = 5*npoin*nlayers
        integer(c_int) function hnumo_stats_fields(eng, out, n) bind(C, name='hnumo_stats_fields')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
        end function hnumo_stats_fields

        ! out(2,nlayers,count) = (KE_k, VOL_k) per sample; n = size(out) >= 2*nlayers*count;
        ! clear = 1 empties the series after the copy
        integer(c_int) function hnumo_stats_series(eng, out, n, count, clear) bind(C, name='hnumo_stats_series')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
            integer(c_int64_t), intent(out) :: count
            integer(c_int32_t), value :: clear
        end function hnumo_stats_series

        integer(c_int) function hnumo_stats_end(eng) bind(C, name='hnumo_stats_end')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_stats_end

        ! Vorticity products on the device state (see include/hnumo_engine.h): zeta, delta, pv, ow from
        ! the element's own gradient of the layer velocity, and the enstrophy / potential-enstrophy /
        ! circulation series, without hnumo_sync.  coriolis_df: c_loc of mod_initial's coriolis_df(npoin),
        ! or c_null_ptr (f = 0).
        integer(c_int) function hnumo_vort_begin(eng, coriolis_df, every, series_capacity) &
                bind(C, name='hnumo_vort_begin')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng, coriolis_df
            integer(c_int32_t), value :: every, series_capacity
        end function hnumo_vort_begin

        ! out(4,npoin,nlayers) = zeta, delta, pv, ow; n = 4*npoin*nlayers
        integer(c_int) function hnumo_vort_fields(eng, out, n) bind(C, name='hnumo_vort_fields')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
        end function hnumo_vort_fields

        integer(c_int) function hnumo_vort_record(eng) bind(C, name='hnumo_vort_record')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_vort_record

        ! out(3,nlayers,count) = (Z_k, PZ_k, G_k) per sample; n = size(out) >= 3*nlayers*count;
        ! clear = 1 empties the series after the copy
        integer(c_int) function hnumo_vort_series(eng, out, n, count, clear) bind(C, name='hnumo_vort_series')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
            integer(c_int64_t), intent(out) :: count
            integer(c_int32_t), value :: clear
        end function hnumo_vort_series

        integer(c_int) function hnumo_vort_end(eng) bind(C, name='hnumo_vort_end')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_vort_end

        ! Eddy covariances on the device state (see include/hnumo_engine.h): Reynolds stresses, eddy
        ! thickness flux, interface / SSH variance, eddy PV flux and eddy potential enstrophy from 14
        ! running sums, without hnumo_sync.  coriolis_df: c_loc of coriolis_df(npoin) or c_null_ptr
        ! (f = 0); zref: c_loc of zref(npoin,nlayers) or c_null_ptr (0).  every = k >= 1: the engine
        ! samples after every k-th successful hnumo_ti_rk_bcl itself.
        integer(c_int) function hnumo_cov_begin(eng, coriolis_df, zref, every) bind(C, name='hnumo_cov_begin')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng, coriolis_df, zref
            integer(c_int32_t), value :: every
        end function hnumo_cov_begin

        integer(c_int) function hnumo_cov_accumulate(eng) bind(C, name='hnumo_cov_accumulate')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_cov_accumulate

        ! out(14,npoin,nlayers) = S_h, S_u, S_v, S_uh, S_vh, S_uuh, S_uvh, S_vvh, S_d, S_dd, S_a, S_ua,
        ! S_va, S_qa; n = 14*npoin*nlayers
        integer(c_int) function hnumo_cov_sums(eng, out, n, nsamples) bind(C, name='hnumo_cov_sums')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
            integer(c_int64_t), intent(out) :: nsamples
        end function hnumo_cov_sums

        integer(c_int) function hnumo_cov_set_sums(eng, sums, n, nsamples) bind(C, name='hnumo_cov_set_sums')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: sums(*)
            integer(c_int64_t), value :: n, nsamples
        end function hnumo_cov_set_sums

        ! out(16,npoin,nlayers) = hbar, ubar, vbar, um, vm, Ruu, Ruv, Rvv, Fu, Fv, dbar, dvar, qm, Qu, Qv,
        ! ens; n = 16*npoin*nlayers
        integer(c_int) function hnumo_cov_fields(eng, out, n) bind(C, name='hnumo_cov_fields')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
        end function hnumo_cov_fields

        ! out(3,nlayers) = the integrals of hbar*(0.5*(Ruu+Rvv)), dvar, hbar*ens; n = 3*nlayers
        integer(c_int) function hnumo_cov_integrals(eng, out, n) bind(C, name='hnumo_cov_integrals')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
        end function hnumo_cov_integrals

        integer(c_int) function hnumo_cov_end(eng) bind(C, name='hnumo_cov_end')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_cov_end

        ! Energy budget on the device state (see include/hnumo_engine.h): wind work and bottom drag at the
        ! quadrature points, interior viscous dissipation at the nodes, with the series of KE, APE, V per
        ! layer and W, D, without hnumo_sync.  zref: c_loc of zref(npoin,nlayers) or c_null_ptr (0).
        ! every = k >= 1: the engine samples after every k-th successful hnumo_ti_rk_bcl itself;
        ! series_capacity: samples the series can hold (0: sums only).
        integer(c_int) function hnumo_energy_begin(eng, zref, every, series_capacity) bind(C, name='hnumo_energy_begin')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng, zref
            integer(c_int32_t), value :: every, series_capacity
        end function hnumo_energy_begin

        integer(c_int) function hnumo_energy_sample(eng) bind(C, name='hnumo_energy_sample')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_energy_sample

        ! out(3*nlayers+2, count) = KE_1..L, APE_1..L, V_1..L, W, D per sample; out: c_loc of the array, or
        ! c_null_ptr for the count alone
        integer(c_int) function hnumo_energy_series(eng, out, n, count, clear) bind(C, name='hnumo_energy_series')
            import :: c_int, c_int32_t, c_int64_t, c_ptr
            type(c_ptr), value :: eng, out
            integer(c_int64_t), value :: n
            integer(c_int64_t), intent(out) :: count
            integer(c_int32_t), value :: clear
        end function hnumo_energy_series

        ! quad2(2,npoin_q) = S_W, S_D, nq2 = 2*npoin_q; nodal(npoin,nlayers) = S_V, nn = npoin*nlayers
        integer(c_int) function hnumo_energy_sums(eng, quad2, nq2, nodal, nn, nsamples) bind(C, name='hnumo_energy_sums')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: quad2(*), nodal(*)
            integer(c_int64_t), value :: nq2, nn
            integer(c_int64_t), intent(out) :: nsamples
        end function hnumo_energy_sums

        integer(c_int) function hnumo_energy_set_sums(eng, quad2, nq2, nodal, nn, nsamples) &
                bind(C, name='hnumo_energy_set_sums')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: quad2(*), nodal(*)
            integer(c_int64_t), value :: nq2, nn, nsamples
        end function hnumo_energy_set_sums

        ! quad2(2,npoin_q) = S_W/N, S_D/N; nodal(npoin,nlayers) = S_V/N: the maps of mean wind power input,
        ! drag and dissipation
        integer(c_int) function hnumo_energy_means(eng, quad2, nq2, nodal, nn) bind(C, name='hnumo_energy_means')
            import :: c_int, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: quad2(*), nodal(*)
            integer(c_int64_t), value :: nq2, nn
        end function hnumo_energy_means

        integer(c_int) function hnumo_energy_end(eng) bind(C, name='hnumo_energy_end')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_energy_end

        ! Region sets (see include/hnumo_engine.h): the integral series of parts of the rank's domain, many
        ! regions reduced at once on the device.  region_of_elem(n), n = nelem_owned, labels 0..nregions (0: in
        ! no region); rows_mask: HNUMO_REGION_FLOW, HNUMO_REGION_VORT or their sum; coriolis_df: c_loc of
        ! coriolis_df(npoin) or c_null_ptr (f = 0).  every = k >= 1: the engine samples after every k-th
        ! successful hnumo_ti_rk_bcl itself; series_capacity: samples the series can hold.
        integer(c_int) function hnumo_regions_create(eng, region_of_elem, n, nregions, rows_mask, coriolis_df, every, &
                series_capacity, id) bind(C, name='hnumo_regions_create')
            import :: c_int, c_int32_t, c_int64_t, c_ptr
            type(c_ptr), value :: eng, coriolis_df
            integer(c_int32_t), intent(in) :: region_of_elem(*)
            integer(c_int64_t), value :: n
            integer(c_int32_t), value :: nregions, rows_mask, every, series_capacity
            integer(c_int32_t), intent(out) :: id
        end function hnumo_regions_create

        integer(c_int) function hnumo_regions_sample(eng, id) bind(C, name='hnumo_regions_sample')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
        end function hnumo_regions_sample

        ! out(V, nregions, count), V = 4*nlayers*[FLOW] + 3*nlayers*[VORT]; out: c_loc of the array, or
        ! c_null_ptr for the count alone
        integer(c_int) function hnumo_regions_series(eng, id, out, n, count, clear) bind(C, name='hnumo_regions_series')
            import :: c_int, c_int32_t, c_int64_t, c_ptr
            type(c_ptr), value :: eng, out
            integer(c_int32_t), value :: id, clear
            integer(c_int64_t), value :: n
            integer(c_int64_t), intent(out) :: count
        end function hnumo_regions_series

        ! out(nregions): the sum of the nodal jac per region
        integer(c_int) function hnumo_regions_area(eng, id, out, n) bind(C, name='hnumo_regions_area')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
        end function hnumo_regions_area

        integer(c_int) function hnumo_regions_destroy(eng, id) bind(C, name='hnumo_regions_destroy')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
        end function hnumo_regions_destroy

        ! Sample sets (see include/hnumo_engine.h): the device state, or the flow statistics, at
        ! arbitrary points by the element's own Lagrange interpolant -- an output grid, a
        ! cross-section, stations -- on demand or after every k-th step into a series on the device.
        ! coord(ldc,npoin) and xgl(ngl) are mod_grid's coord and mod_basis' xgl; xy(2,M) the points.
        integer(c_int) function hnumo_sample_create(eng, coord, ldc, xgl, xy, M, source, id) &
                bind(C, name='hnumo_sample_create')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: coord(*), xgl(*), xy(*)
            integer(c_int32_t), value :: ldc, source
            integer(c_int64_t), value :: M
            integer(c_int32_t), intent(out) :: id
        end function hnumo_sample_create

        ! elem(M): 1-based local element, 0 = not on this rank; xi_eta(2,M) in [-1,1]
        integer(c_int) function hnumo_sample_create_ref(eng, xgl, elem, xi_eta, M, source, id) &
                bind(C, name='hnumo_sample_create_ref')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: xgl(*), xi_eta(*)
            integer(c_int32_t), intent(in) :: elem(*)
            integer(c_int64_t), value :: M
            integer(c_int32_t), value :: source
            integer(c_int32_t), intent(out) :: id
        end function hnumo_sample_create_ref

        integer(c_int) function hnumo_sample_plan(eng, id, elem, xi_eta, M) bind(C, name='hnumo_sample_plan')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            integer(c_int32_t), intent(out) :: elem(*)
            real(c_double), intent(out) :: xi_eta(*)
            integer(c_int64_t), value :: M
        end function hnumo_sample_plan

        ! out(V,M), n = V*M; V = 5*nlayers + 4 (HNUMO_SAMPLE_STATE), 5*nlayers (HNUMO_SAMPLE_STATS) or
        ! 4*nlayers (HNUMO_SAMPLE_VORT) or 16*nlayers (HNUMO_SAMPLE_COV)
        integer(c_int) function hnumo_sample(eng, id, out, n) bind(C, name='hnumo_sample')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
        end function hnumo_sample

        integer(c_int) function hnumo_sample_series_begin(eng, id, every, capacity) &
                bind(C, name='hnumo_sample_series_begin')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id, every, capacity
        end function hnumo_sample_series_begin

        integer(c_int) function hnumo_sample_record(eng, id) bind(C, name='hnumo_sample_record')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
        end function hnumo_sample_record

        ! out(V,M,count); n = size(out) >= V*M*count; clear = 1 empties the series after the copy
        integer(c_int) function hnumo_sample_series(eng, id, out, n, count, clear) bind(C, name='hnumo_sample_series')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
            integer(c_int64_t), intent(out) :: count
            integer(c_int32_t), value :: clear
        end function hnumo_sample_series

        integer(c_int) function hnumo_sample_destroy(eng, id) bind(C, name='hnumo_sample_destroy')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
        end function hnumo_sample_destroy

        ! Float sets (see include/hnumo_engine.h): Lagrangian floats that live in a layer and move with
        ! its velocity, advanced on the device after every step.  coord(ldc,npoin) and xgl(ngl) are
        ! mod_grid's coord and mod_basis' xgl; xy(2,M) the seeds, layer(M) in 1..nlayers.
        integer(c_int) function hnumo_floats_create(eng, coord, ldc, xgl, xy, layer, M, id) &
                bind(C, name='hnumo_floats_create')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: coord(*), xgl(*), xy(*)
            integer(c_int32_t), intent(in) :: layer(*)
            integer(c_int32_t), value :: ldc
            integer(c_int64_t), value :: M
            integer(c_int32_t), intent(out) :: id
        end function hnumo_floats_create

        ! x, y, u, v, elem, status (M each) in input order; status HNUMO_FLOAT_ACTIVE / LEFT / LOST
        integer(c_int) function hnumo_floats_get(eng, id, x, y, u, v, elem, status, M) bind(C, name='hnumo_floats_get')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            real(c_double), intent(out) :: x(*), y(*), u(*), v(*)
            integer(c_int32_t), intent(out) :: elem(*), status(*)
            integer(c_int64_t), value :: M
        end function hnumo_floats_get

        ! the cached locations elem(M), xi_eta(2,M) in input order
        integer(c_int) function hnumo_floats_plan(eng, id, elem, xi_eta, M) bind(C, name='hnumo_floats_plan')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            integer(c_int32_t), intent(out) :: elem(*)
            real(c_double), intent(out) :: xi_eta(*)
            integer(c_int64_t), value :: M
        end function hnumo_floats_plan

        integer(c_int) function hnumo_floats_set(eng, id, xy, layer, M) bind(C, name='hnumo_floats_set')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            real(c_double), intent(in) :: xy(*)
            integer(c_int32_t), intent(in) :: layer(*)
            integer(c_int64_t), value :: M
        end function hnumo_floats_set

        integer(c_int) function hnumo_floats_advance(eng, id, dt) bind(C, name='hnumo_floats_advance')
            import :: c_int, c_int32_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            real(c_double), value :: dt
        end function hnumo_floats_advance

        ! every = 1: the engine advances the set by dt after every successful step; a record after every
        ! record_every-th advance into a series of `capacity` records on the device
        integer(c_int) function hnumo_floats_begin(eng, id, every, record_every, capacity) &
                bind(C, name='hnumo_floats_begin')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id, every, record_every, capacity
        end function hnumo_floats_begin

        integer(c_int) function hnumo_floats_record(eng, id) bind(C, name='hnumo_floats_record')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
        end function hnumo_floats_record

        ! out(5,M,count) = x, y, u, v, elem; n = size(out) >= 5*M*count; clear = 1 empties the series
        integer(c_int) function hnumo_floats_series(eng, id, out, n, count, clear) bind(C, name='hnumo_floats_series')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
            integer(c_int64_t), intent(out) :: count
            integer(c_int32_t), value :: clear
        end function hnumo_floats_series

        integer(c_int) function hnumo_floats_destroy(eng, id) bind(C, name='hnumo_floats_destroy')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
        end function hnumo_floats_destroy

        ! migrating sets (processor-face ranks): on = 1 hands floats that reach a processor face to the rank
        ! across it; coord_scale > 0 replaces the rank's max|coord| in tol_e
        integer(c_int) function hnumo_floats_migrate(eng, id, on, coord_scale) bind(C, name='hnumo_floats_migrate')
            import :: c_int, c_int32_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id, on
            real(c_double), value :: coord_scale
        end function hnumo_floats_migrate

        ! floats idx(n) (0-based input positions) that are ACTIVE on this rank become LEFT
        integer(c_int) function hnumo_floats_release(eng, id, idx, n) bind(C, name='hnumo_floats_release')
            import :: c_int, c_int32_t, c_int64_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            integer(c_int32_t), intent(in) :: idx(*)
            integer(c_int64_t), value :: n
        end function hnumo_floats_release

        ! d(cap,7) = x, y, wx, wy, dt, px, py; i(cap,6) = gid, layer, stage, hops, dest (0-based rank), pos
        integer(c_int) function hnumo_floats_outbox(eng, id, d, i, cap, count) bind(C, name='hnumo_floats_outbox')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            real(c_double), intent(out) :: d(*)
            integer(c_int32_t), intent(out) :: i(*)
            integer(c_int64_t), value :: cap
            integer(c_int64_t), intent(out) :: count
        end function hnumo_floats_outbox

        integer(c_int) function hnumo_floats_deliver(eng, id, src_rank, d, i, cap, n) bind(C, name='hnumo_floats_deliver')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id, src_rank
            real(c_double), intent(in) :: d(*)
            integer(c_int32_t), intent(in) :: i(*)
            integer(c_int64_t), value :: cap, n
        end function hnumo_floats_deliver

        integer(c_int) function hnumo_floats_settle(eng, id) bind(C, name='hnumo_floats_settle')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
        end function hnumo_floats_settle

        ! sensors: mask = HNUMO_FLOAT_SENSE_STATE + HNUMO_FLOAT_SENSE_VORT adds S = 5 + 4 rows (h, u, v, dp, elevation;
        ! zeta, delta, pv, ow of the float's own layer) to every record: hnumo_floats_series then returns out(5+S,M,count).
        ! Sensors first, then hnumo_floats_begin
        integer(c_int) function hnumo_floats_sensors(eng, id, mask) bind(C, name='hnumo_floats_sensors')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id, mask
        end function hnumo_floats_sensors

        ! out(S,M) in input order: the sensors on the state on the device now; n = S*M
        integer(c_int) function hnumo_floats_sense(eng, id, out, n) bind(C, name='hnumo_floats_sense')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            real(c_double), intent(out) :: out(*)
            integer(c_int64_t), value :: n
        end function hnumo_floats_sense

        ! nrows = S; K = the element slots of the sensor kernel's arena for this set (0 without sensors)
        integer(c_int) function hnumo_floats_sense_info(eng, id, nrows, K) bind(C, name='hnumo_floats_sense_info')
            import :: c_int, c_int32_t, c_ptr
            type(c_ptr), value :: eng
            integer(c_int32_t), value :: id
            integer(c_int32_t), intent(out) :: nrows, K
        end function hnumo_floats_sense_info

        ! ---- time-dependent wind stress (hnumo_wind_*, include/hnumo_engine.h): the wind as a linear
        ! combination of M <= HNUMO_WIND_MAXM patterns, formed on the device
        ! patterns(2,npoin_q,M), n = size(patterns); the wind is unchanged until a set or a scheduled step
        integer(c_int) function hnumo_wind_begin(eng, patterns, n, M) bind(C, name='hnumo_wind_begin')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: patterns(*)
            integer(c_int64_t), value :: n
            integer(c_int32_t), value :: M
        end function hnumo_wind_begin

        ! tau_wind = coef(1)*T_1 + ... + coef(M)*T_M now, for every later step
        integer(c_int) function hnumo_wind_set(eng, coef, M) bind(C, name='hnumo_wind_set')
            import :: c_int, c_int32_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: coef(*)
            integer(c_int32_t), value :: M
        end function hnumo_wind_set

        ! coef(M,nrows) copied to the device once; the k-th successful step since this call uses row
        ! first + k (0-based), held at the last row (HNUMO_WIND_HOLD) or taken modulo nrows (HNUMO_WIND_REPEAT)
        integer(c_int) function hnumo_wind_schedule(eng, coef, M, nrows, first, mode) bind(C, name='hnumo_wind_schedule')
            import :: c_int, c_int32_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(in) :: coef(*)
            integer(c_int32_t), value :: M, nrows, first, mode
        end function hnumo_wind_schedule

        ! tau(2,npoin_q), n = size(tau): the current wind; next_row: the row the next step uses (-1: none)
        integer(c_int) function hnumo_wind_get(eng, tau, n, next_row) bind(C, name='hnumo_wind_get')
            import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double
            type(c_ptr), value :: eng
            real(c_double), intent(out) :: tau(*)
            integer(c_int64_t), value :: n
            integer(c_int32_t), intent(out) :: next_row
        end function hnumo_wind_get

        ! the create-time wind again, bit for bit
        integer(c_int) function hnumo_wind_end(eng) bind(C, name='hnumo_wind_end')
            import :: c_int, c_ptr
            type(c_ptr), value :: eng
        end function hnumo_wind_end
    end interface

contains

    ! hnumo_last_error() as a Fortran string
    function hnumo_last_error(eng) result(msg)
        type(c_ptr), intent(in) :: eng
        character(len=:), allocatable :: msg
        character(kind=c_char), pointer :: s(:)
        integer :: n
        call c_f_pointer(hnumo_last_error_c(eng), s, [4096])
        n = 0
        do while (n < 4096)
            if (s(n + 1) == c_null_char) exit
            n = n + 1
        end do
        allocate(character(len=n) :: msg)
        msg = transfer(s(1:n), msg)
    end function hnumo_last_error

    ! copy out a mod_variables equivalent by name, e.g. call hnumo_get_field(eng, 'H_ave', H_ave, rc)
    subroutine hnumo_get_field(eng, name, out, rc)
        type(c_ptr), intent(in) :: eng
        character(len=*), intent(in) :: name
        real(c_double), intent(out) :: out(:)
        integer(c_int), intent(out) :: rc
        rc = hnumo_get_field_c(eng, trim(name) // c_null_char, out, int(size(out), c_int64_t))
    end subroutine hnumo_get_field

end module hnumo_engine_c
