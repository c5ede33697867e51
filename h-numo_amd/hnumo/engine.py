"""Python host mirror of the reference's engine boundary (ti_rk_bcl and its parity hooks)
over the C ABI of libhnumo_engine.so (include/hnumo_engine.h).

The product path is the HIP library; there is no CPU fallback.  Loading fails loudly if
the library is missing or no GPU is visible.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi
from . import bundle as _bundle
from .abi import Descriptors, Halo, HaloDesc

LIB_PATH = os.environ.get("HNUMO_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                    "libhnumo_engine.so")  # HNUMO_LIB: A/B experiments only
_lib = None

ERRORS = {1: "negative layer thickness", 2: "non-finite value", 3: "HIP/RCCL error", 4: "invalid argument"}


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hnumo engine error {code} ({ERRORS.get(code, '?')}): {msg}")
        self.code = code


def lib():
    """Load libhnumo_engine.so (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        vp, dp = C.c_void_p, C.POINTER(C.c_double)
        L.hnumo_engine_create.argtypes = [vp, vp, vp, vp, C.c_int, C.POINTER(vp)]
        L.hnumo_engine_destroy.argtypes = [vp]
        L.hnumo_last_error.argtypes = [vp]
        L.hnumo_last_error.restype = C.c_char_p
        L.hnumo_ti_rk_bcl.argtypes = [vp, dp, dp, dp]
        L.hnumo_ti_barotropic_ssprk.argtypes = [vp, dp, dp]
        L.hnumo_predict.argtypes = [vp, dp, dp, dp]
        L.hnumo_btp_bcl_coeffs.argtypes = [vp, dp]
        L.hnumo_create_rhs_btp.argtypes = [vp, dp, dp, dp]
        L.hnumo_get_field.argtypes = [vp, C.c_char_p, dp, C.c_int64]
        L.hnumo_set_resident.argtypes = [vp, C.c_int]
        L.hnumo_sync.argtypes = [vp, dp, dp, dp]
        L.hnumo_bench_steps.argtypes = [vp, C.c_int, dp, dp, C.POINTER(C.c_int64)]
        L.hnumo_abi_version.restype = C.c_int
        L.hnumo_time_stage_kernel.argtypes = [vp, C.c_int, dp]
        L.hnumo_rccl_unique_id.argtypes = [C.POINTER(C.c_ubyte)]
        L.hnumo_local_group.argtypes = [C.POINTER(vp), C.c_int]
        L.hnumo_group_ti_rk_bcl.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(dp), C.POINTER(dp), C.POINTER(dp)]
        L.hnumo_debug_stage_profile.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int64]
        L.hnumo_set_summation.argtypes = [vp, C.c_int]
        L.hnumo_get_summation.argtypes = [vp]
        L.hnumo_get_summation.restype = C.c_int
        L.hnumo_stage_path.argtypes = [vp]
        L.hnumo_stage_path.restype = C.c_int
        L.hnumo_kernel_variants.argtypes = [vp, C.POINTER(C.c_int32)]
        L.hnumo_persistent_info.argtypes = [vp, C.POINTER(C.c_int32)]
        L.hnumo_persistent_stats.argtypes = [vp, C.POINTER(C.c_int32)]
        L.hnumo_debug_force_abort.argtypes = [vp, C.c_int]
        L.hnumo_debug_frozen_halo.argtypes = [vp, C.c_int]
        L.hnumo_step_breakdown.argtypes = [vp, C.c_int, C.c_char_p, C.c_int64, dp, C.c_int, C.POINTER(C.c_int)]
        L.hnumo_stream_copy_bw.argtypes = [C.c_int, C.c_int64, C.c_int, dp]
        L.hnumo_overrides.argtypes = [vp, C.c_char_p, C.c_int64]
        L.hnumo_diag_geometry.argtypes = [vp, dp, C.c_int32, dp]
        L.hnumo_diagnostics.argtypes = [vp, C.c_int32, dp, C.c_int64]
        L.hnumo_layer_fields.argtypes = [vp, dp, C.c_int64]
        L.hnumo_stats_begin.argtypes = [vp, C.c_int32, C.c_int32]
        L.hnumo_stats_accumulate.argtypes = [vp]
        L.hnumo_stats_sums.argtypes = [vp, dp, C.c_int64, C.POINTER(C.c_int64)]
        L.hnumo_stats_set_sums.argtypes = [vp, dp, C.c_int64, C.c_int64]
        L.hnumo_stats_fields.argtypes = [vp, dp, C.c_int64]
        L.hnumo_stats_series.argtypes = [vp, dp, C.c_int64, C.POINTER(C.c_int64), C.c_int32]
        L.hnumo_stats_end.argtypes = [vp]
        L.hnumo_vort_begin.argtypes = [vp, dp, C.c_int32, C.c_int32]
        L.hnumo_vort_fields.argtypes = [vp, dp, C.c_int64]
        L.hnumo_vort_record.argtypes = [vp]
        L.hnumo_vort_series.argtypes = [vp, dp, C.c_int64, C.POINTER(C.c_int64), C.c_int32]
        L.hnumo_vort_end.argtypes = [vp]
        ip, i32, i64 = C.POINTER(C.c_int32), C.c_int32, C.c_int64
        L.hnumo_sample_create.argtypes = [vp, dp, i32, dp, dp, i64, i32, ip]
        L.hnumo_sample_create_ref.argtypes = [vp, dp, ip, dp, i64, i32, ip]
        L.hnumo_sample_plan.argtypes = [vp, i32, ip, dp, i64]
        L.hnumo_sample.argtypes = [vp, i32, dp, i64]
        L.hnumo_sample_series_begin.argtypes = [vp, i32, i32, i32]
        L.hnumo_sample_record.argtypes = [vp, i32]
        L.hnumo_sample_series.argtypes = [vp, i32, dp, i64, C.POINTER(i64), i32]
        L.hnumo_sample_destroy.argtypes = [vp, i32]
        L.hnumo_floats_create.argtypes = [vp, dp, i32, dp, dp, ip, i64, ip]
        L.hnumo_floats_get.argtypes = [vp, i32, dp, dp, dp, dp, ip, ip, i64]
        L.hnumo_floats_plan.argtypes = [vp, i32, ip, dp, i64]
        L.hnumo_floats_set.argtypes = [vp, i32, dp, ip, i64]
        L.hnumo_floats_advance.argtypes = [vp, i32, C.c_double]
        L.hnumo_floats_begin.argtypes = [vp, i32, i32, i32, i32]
        L.hnumo_floats_record.argtypes = [vp, i32]
        L.hnumo_floats_series.argtypes = [vp, i32, dp, i64, C.POINTER(i64), i32]
        L.hnumo_floats_destroy.argtypes = [vp, i32]
        L.hnumo_floats_migrate.argtypes = [vp, i32, i32, C.c_double]
        L.hnumo_floats_release.argtypes = [vp, i32, ip, i64]
        L.hnumo_floats_outbox.argtypes = [vp, i32, dp, ip, i64, C.POINTER(i64)]
        L.hnumo_floats_deliver.argtypes = [vp, i32, i32, dp, ip, i64, i64]
        L.hnumo_floats_settle.argtypes = [vp, i32]
        L.hnumo_group_floats_migrate.argtypes = [C.POINTER(vp), C.c_int, i32, i32, C.c_double]
        L.hnumo_group_floats_advance.argtypes = [C.POINTER(vp), C.c_int, i32, C.c_double]
        abi.declare_float_sensors(L)
        abi.declare_cov(L)
        abi.declare_energy(L)
        abi.declare_regions(L)
        L.hnumo_wind_begin.argtypes = [vp, dp, i64, i32]
        L.hnumo_wind_set.argtypes = [vp, dp, i32]
        L.hnumo_wind_schedule.argtypes = [vp, dp, i32, i32, i32, i32]
        L.hnumo_wind_get.argtypes = [vp, dp, i64, ip]
        L.hnumo_wind_end.argtypes = [vp]
        _lib = L
    return _lib


def _dp(a, size=None, name="array"):
    """Pointer to a float64 Fortran-contiguous array of exactly `size` elements (the C side
    reads and writes fixed-size blocks, so a wrong shape must never reach it)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags["F_CONTIGUOUS"]:
        raise ValueError(f"{name}: need a Fortran-contiguous float64 numpy array")
    if not a.flags["WRITEABLE"]:
        raise ValueError(f"{name}: array is read-only")
    if size is not None and a.size != size:
        raise ValueError(f"{name}: {a.size} elements, expected {size}")
    return a.ctypes.data_as(C.POINTER(C.c_double))


SUMMATION = {"reference": 0, "factored": 1}   # HNUMO_SUM_REFERENCE / HNUMO_SUM_FACTORED
DIAG_MASS = 1                                 # HNUMO_DIAG_MASS
SAMPLE_STATE, SAMPLE_STATS = 0, 1             # HNUMO_SAMPLE_STATE / HNUMO_SAMPLE_STATS
SAMPLE_VORT = 2                               # HNUMO_SAMPLE_VORT
SAMPLE_COV = 3                                # HNUMO_SAMPLE_COV


def unpack_diagnostics(out, L: int) -> dict:
    """hnumo_diagnostics' flat out array (12 + 11*L values: [cfl_b, cfl, min_dx, min_dy,
    qbmax(4), qbmin(4)], then per layer [mass, qmax(5), qmin(5)]) as a dict; qmax/qmin are
    (5, L) as print_diagnostics uses them, mass is (L,)."""
    out = np.asarray(out, dtype=np.float64).reshape(-1)
    if out.size != 12 + 11 * L:
        raise ValueError(f"diagnostics: {out.size} values, expected 12 + 11*{L} = {12 + 11 * L}")
    lay = out[12:].reshape(L, 11)
    return {"cfl_b": float(out[0]), "cfl": float(out[1]), "min_dx": float(out[2]), "min_dy": float(out[3]),
            "qbmax": out[4:8].copy(), "qbmin": out[8:12].copy(), "mass": lay[:, 0].copy(),
            "qmax": np.ascontiguousarray(lay[:, 1:6].T), "qmin": np.ascontiguousarray(lay[:, 6:11].T)}


class Engine:
    """One engine per GPU: device-resident ti_rk_bcl for one Case."""

    def __init__(self, case, device: int = 0, halo: HaloDesc | None = None, comm_id: bytes | None = None,
                 summation: str | None = None):
        """case: a hnumo.case.Case, or a hnumo.partition.RankCase (multi-rank; its ghost-layer
        halo is passed to the engine, with RCCL when comm_id is given).  summation:
        "reference" (the default: bit-identical to the reference order) or "factored"
        (sum-factorised, faster, ~1e-7 relative from the reference; see hnumo_set_summation)."""
        self.case = case
        self.desc = Descriptors(case, dense=False)
        self.dims = _bundle.dims(case)
        self.h = C.c_void_p()
        if halo is None and (getattr(case, "nranks", 1) > 1 or getattr(case, "fneighbours", None)):
            self._halo = Halo(case, comm_id)
            halo = self._halo.desc
        self.halo = halo
        L = lib()
        rc = L.hnumo_engine_create(C.byref(self.desc.mesh), C.byref(self.desc.statics), C.byref(self.desc.params),
                                   C.byref(halo) if halo is not None else None, device, C.byref(self.h))
        if rc:
            msg = L.hnumo_last_error(self.h).decode()
            self._destroy()
            raise EngineError(rc, msg)
        if summation is not None:
            self.set_summation(summation)
        if "coord" in case.arrays:
            try:
                self.diag_geometry(case.arrays["coord"], case.arrays.get("wjac_df"))
            except EngineError:
                self._destroy()
                raise

    def _check(self, rc):
        if rc:
            raise EngineError(rc, lib().hnumo_last_error(self.h).decode())

    def state(self):
        A = self.case.arrays
        return (np.array(A["q_df"], order="F"), np.array(A["qb_df"], order="F"),
                np.array(A["qprime_df"], order="F"))

    # sizes of q_df(3,npoin,L), qb_df(4,npoin), qprime_df(3,npoin,L)
    def _sizes(self):
        d = self.dims
        return 3 * d["npoin"] * d["nlayers"], 4 * d["npoin"], 3 * d["npoin"] * d["nlayers"]

    def _state_ptrs(self, q, qb, qp):
        nq, nb, np_ = self._sizes()
        return _dp(q, nq, "q_df"), _dp(qb, nb, "qb_df"), _dp(qp, np_, "qprime_df")

    # = ti_rk_bcl (ti_rk_bcl.F90:9)
    def ti_rk_bcl(self, q, qb, qp):
        self._check(lib().hnumo_ti_rk_bcl(self.h, *self._state_ptrs(q, qb, qp)))

    # = the prediction half of ti_rk_bcl (ti_rk_bcl.F90:43-57): q, qb, qp become q_df2, the
    # sub-cycled qb_df and qprime_df2
    def predict(self, q, qb, qp):
        self._check(lib().hnumo_predict(self.h, *self._state_ptrs(q, qb, qp)))

    def btp_bcl_coeffs(self, qp):
        self._check(lib().hnumo_btp_bcl_coeffs(self.h, _dp(qp, self._sizes()[2], "qprime_df")))

    # = ti_barotropic_ssprk_mlswe (mod_rk_mlswe.F90:19)
    def ti_barotropic_ssprk(self, qb, qp):
        _, nb, np_ = self._sizes()
        self._check(lib().hnumo_ti_barotropic_ssprk(self.h, _dp(qb, nb, "qb_df"), _dp(qp, np_, "qprime_df")))

    # = create_rhs_btp (mod_rhs_btp.F90:28)
    def create_rhs_btp(self, qb, qp):
        _, nb, np_ = self._sizes()
        rhs = np.zeros((3, self.dims["npoin"]), order="F")
        self._check(lib().hnumo_create_rhs_btp(self.h, _dp(rhs), _dp(qb, nb, "qb_df"), _dp(qp, np_, "qprime_df")))
        return rhs

    def field(self, name):
        shp = dict(_bundle.FIELDS)[name]
        out = np.zeros(_bundle.shape_of(shp, self.dims), order="F")
        self._check(lib().hnumo_get_field(self.h, name.encode(), _dp(out), out.size))
        return out

    def set_summation(self, mode: str):
        self._check(lib().hnumo_set_summation(self.h, SUMMATION[mode]))

    @property
    def summation(self) -> str:
        return {v: k for k, v in SUMMATION.items()}[lib().hnumo_get_summation(self.h)]

    @property
    def stage_path(self) -> str:
        """'persistent' (one launch per sub-cycle) or 'per-stage' (one launch per stage)."""
        return "persistent" if lib().hnumo_stage_path(self.h) == 1 else "per-stage"

    @property
    def kernel_variants(self) -> dict:
        """The device code variants this engine launches (hnumo_kernel_variants): stage_arena, the
        per-stage barotropic kernel's LDS arena (5 or 4: a LEAN arena of large meshes, 0: the
        small-mesh arena, and always 0 unless N = 4 in the reference summation order), and bcl_big,
        whether the layer mass / consistency kernels are the large-mesh ones."""
        out = (C.c_int32 * 2)()
        self._check(lib().hnumo_kernel_variants(self.h, out))
        return dict(stage_arena=int(out[0]), bcl_big=bool(out[1]))

    @property
    def persistent_info(self) -> dict:
        """Residency of the persistent sub-cycle launch (hnumo_persistent_info)."""
        out = (C.c_int32 * 8)()
        self._check(lib().hnumo_persistent_info(self.h, out))
        v = list(out)
        return {"persistent": v[0] == 1, "occupancy_blocks_per_cu": (v[1], v[2]), "cus": v[3],
                "trial_launch": (v[4], v[5]), "fallbacks": v[6], "lds_bytes_per_workgroup": v[7]}

    @property
    def persistent_stats(self) -> dict:
        """The persistent path's in-launch residency check over the engine's life
        (hnumo_persistent_stats): launches that gave up, trial re-probes, re-probes that found the
        grid resident again, and the runs left before the next re-probe (-1: not suspended)."""
        out = (C.c_int32 * 4)()
        self._check(lib().hnumo_persistent_stats(self.h, out))
        v = list(out)
        return {"aborts": v[0], "reprobes": v[1], "recovered": v[2], "wait": v[3]}

    @property
    def overrides(self) -> list:
        """The HNUMO_* environment settings this engine read at create (hnumo_overrides):
        "NAME=value", with " (ignored: HNUMO_EXPERIMENTS!=1)" for experiment knobs not honoured."""
        buf = C.create_string_buffer(4096)
        self._check(lib().hnumo_overrides(self.h, buf, len(buf)))
        return [x for x in buf.value.decode().split(";") if x]

    def debug_force_abort(self, k: int):
        """Test hook: the k-th persistent sub-cycle launch from now (0 = the next) gives up as a
        launch whose workgroups are not co-resident does (hnumo_debug_force_abort)."""
        self._check(lib().hnumo_debug_force_abort(self.h, int(k)))

    def debug_frozen_halo(self, on: bool = True):
        """Emulation hook (self-neighbour engines only, bench.py --emulate): every halo exchange
        site sends its first message again and again -- an at-rest neighbour for an at-rest case
        (hnumo_debug_frozen_halo).  Set before the first step."""
        self._check(lib().hnumo_debug_frozen_halo(self.h, int(on)))

    def set_resident(self, on: bool):
        self._check(lib().hnumo_set_resident(self.h, int(on)))

    def sync(self, q, qb, qp):
        self._check(lib().hnumo_sync(self.h, *self._state_ptrs(q, qb, qp)))

    # ---- run diagnostics on the device state (hnumo_diag_geometry / hnumo_diagnostics)
    def diag_geometry(self, coord, wjac_df=None):
        """The grid data of diagnostics(): coord(2 or 3, npoin) = mod_grid coord and, optionally,
        wjac_df(npoin) (default: the nodal jac of the case).  Engine() calls it when the case
        carries `coord`."""
        npoin = self.dims["npoin"]
        coord = np.asfortranarray(coord, dtype=np.float64)
        if coord.ndim != 2 or coord.shape[1] != npoin:
            raise ValueError(f"coord: shape {coord.shape}, expected (2 or 3, {npoin})")
        cp = coord.ctypes.data_as(C.POINTER(C.c_double))
        wp = None
        if wjac_df is not None:
            w = np.ascontiguousarray(np.asarray(wjac_df, dtype=np.float64).reshape(-1, order="F"))
            if w.size != npoin:
                raise ValueError(f"wjac_df: {w.size} elements, expected {npoin}")
            wp = w.ctypes.data_as(C.POINTER(C.c_double))
        self._check(lib().hnumo_diag_geometry(self.h, cp, coord.shape[0], wp))

    def diagnostics(self, mass: bool = True) -> dict:
        """The reference's run diagnostics (print_diagnostics.F90) of the state on the device,
        computed there: no sync.  Keys cfl_b, cfl, min_dx, min_dy, qbmax, qbmin (4), mass (L; zeros
        with mass=False, which skips the one sequential sum), qmax, qmin (5, L)."""
        L = self.dims["nlayers"]
        out = np.zeros(12 + 11 * L)
        self._check(lib().hnumo_diagnostics(self.h, DIAG_MASS if mass else 0, _dp(out), out.size))
        return unpack_diagnostics(out, L)

    def layer_fields(self):
        """q(5,npoin,nlayers) of diagnostics.F90:24-45 for the state on the device."""
        out = np.zeros((5, self.dims["npoin"], self.dims["nlayers"]), order="F")
        self._check(lib().hnumo_layer_fields(self.h, _dp(out), out.size))
        return out

    # ---- what the observers below share
    def _series(self, fn, head_shape, *ids, clear=False):
        """(*head_shape, count) of a series: the (NULL, 0) query for the count, then the read."""
        n = C.c_int64()
        self._check(fn(self.h, *ids, None, 0, C.byref(n), 0))
        out = np.zeros((*head_shape, n.value), order="F")
        if n.value or clear:
            buf = out if out.size else np.zeros(1)
            self._check(fn(self.h, *ids, _dp(buf), out.size, C.byref(n), int(clear)))
        return out

    def _plan(self, fn, sid: int, M: int):
        elem = np.zeros(M, dtype=np.int32)
        xe = np.zeros((2, M), order="F")
        self._check(fn(self.h, int(sid), elem.ctypes.data_as(C.POINTER(C.c_int32)), _dp(xe), M))
        return elem, xe

    def _coord_arg(self, coord):
        coord = np.asfortranarray(coord, dtype=np.float64)
        if coord.ndim != 2 or coord.shape[1] != self.dims["npoin"]:
            raise ValueError(f"coord: shape {coord.shape}, expected (2 or 3, {self.dims['npoin']})")
        return coord

    @staticmethod
    def _xy_arg(xy):
        xy = np.asfortranarray(xy, dtype=np.float64)
        if xy.ndim != 2 or xy.shape[0] != 2:
            raise ValueError(f"xy: shape {xy.shape}, expected (2, M)")
        return xy

    def _sets(self, kind: str) -> dict:
        """id -> sizes of the `kind` ("sample": (M, V); "float": M) sets created through this object."""
        return self.__dict__.setdefault("_sets_", {}).setdefault(kind, {})

    def _set_sizes(self, kind: str, sid: int):
        if sid not in self._sets(kind):
            raise EngineError(4, f"no {kind} set with id {sid}")
        return self._sets(kind)[sid]

    # ---- online flow statistics on the device state (hnumo_stats_*; mirror: hnumo/flowstats.py)
    def stats_begin(self, every: int = 0, series: int = 0):
        """Allocate and zero the running sums (again: reset).  every = k >= 1: the engine samples
        itself after every k-th successful step; series: samples the KE/VOL series can hold (0: none)."""
        self._check(lib().hnumo_stats_begin(self.h, int(every), int(series)))

    def stats_accumulate(self):
        """One sample of the state on the device; nothing is copied back."""
        self._check(lib().hnumo_stats_accumulate(self.h))

    def stats_sums(self):
        """(sums (4, npoin, nlayers) = S_h, S_uh, S_vh, S_e; the sample count)."""
        out = np.zeros((4, self.dims["npoin"], self.dims["nlayers"]), order="F")
        n = C.c_int64()
        self._check(lib().hnumo_stats_sums(self.h, _dp(out), out.size, C.byref(n)))
        return out, n.value

    def stats_set_sums(self, sums, nsamples: int):
        """Restore sums (4, npoin, nlayers) and a sample count, e.g. of a run being restarted."""
        a = np.array(sums, dtype=np.float64, order="F")
        size = 4 * self.dims["npoin"] * self.dims["nlayers"]
        self._check(lib().hnumo_stats_set_sums(self.h, _dp(a, size, "sums"), a.size, int(nsamples)))

    def stats_fields(self):
        """(5, npoin, nlayers) = hbar, um, vm, mke, eke of the samples so far."""
        out = np.zeros((5, self.dims["npoin"], self.dims["nlayers"]), order="F")
        self._check(lib().hnumo_stats_fields(self.h, _dp(out), out.size))
        return out

    def stats_series(self, clear: bool = False):
        """(2, nlayers, count) = (KE_k, VOL_k) per sample; clear empties the series afterwards."""
        return self._series(lib().hnumo_stats_series, (2, self.dims["nlayers"]), clear=clear)

    def stats_end(self):
        self._check(lib().hnumo_stats_end(self.h))

    # ---- vorticity products of the device state (hnumo_vort_*; mirror: hnumo/vorticity.py)
    def vort_begin(self, coriolis_df=None, every: int = 0, series: int = 0):
        """Allocate the buffers (again: reset).  coriolis_df (npoin), or None: f = 0.  every = k >= 1:
        the engine takes a series sample itself after every k-th successful step; series: samples the
        series can hold (0: none)."""
        fp = None
        if coriolis_df is not None:
            f = np.ascontiguousarray(np.asarray(coriolis_df, dtype=np.float64).reshape(-1))
            if f.size != self.dims["npoin"]:
                raise ValueError(f"coriolis_df: {f.size} elements, expected {self.dims['npoin']}")
            fp = f.ctypes.data_as(C.POINTER(C.c_double))
        self._check(lib().hnumo_vort_begin(self.h, fp, int(every), int(series)))

    def vort_fields(self):
        """(4, npoin, nlayers) = zeta, delta, pv, ow of the state on the device now."""
        out = np.zeros((4, self.dims["npoin"], self.dims["nlayers"]), order="F")
        self._check(lib().hnumo_vort_fields(self.h, _dp(out), out.size))
        return out

    def vort_record(self):
        """Append one series sample on the device; nothing is copied back."""
        self._check(lib().hnumo_vort_record(self.h))

    def vort_series(self, clear: bool = False):
        """(3, nlayers, count) = (Z_k, PZ_k, G_k) per sample; clear empties the series afterwards."""
        return self._series(lib().hnumo_vort_series, (3, self.dims["nlayers"]), clear=clear)

    def vort_end(self):
        self._check(lib().hnumo_vort_end(self.h))

    # ---- eddy covariances of the device state (hnumo_cov_*; mirror: hnumo/covariance.py)
    def cov_begin(self, coriolis_df=None, zref=None, every: int = 0):
        """Allocate and zero the running sums (again: reset).  coriolis_df (npoin), or None: f = 0; zref
        (npoin, nlayers), or None: 0.  every = k >= 1: the engine samples itself after every k-th
        successful step."""
        npoin, L = self.dims["npoin"], self.dims["nlayers"]
        fp = zp = None
        if coriolis_df is not None:
            f = np.ascontiguousarray(np.asarray(coriolis_df, dtype=np.float64).reshape(-1))
            if f.size != npoin:
                raise ValueError(f"coriolis_df: {f.size} elements, expected {npoin}")
            fp = f.ctypes.data_as(C.POINTER(C.c_double))
        if zref is not None:
            z = np.array(zref, dtype=np.float64, order="F")
            if z.shape != (npoin, L):
                raise ValueError(f"zref: shape {z.shape}, expected (npoin, nlayers) = ({npoin}, {L})")
            zp = z.ctypes.data_as(C.POINTER(C.c_double))
        self._check(lib().hnumo_cov_begin(self.h, fp, zp, int(every)))

    def cov_accumulate(self):
        """One sample of the state on the device; nothing is copied back."""
        self._check(lib().hnumo_cov_accumulate(self.h))

    def cov_sums(self):
        """(sums (14, npoin, nlayers) in the order of covariance.SUM_NAMES; the sample count)."""
        out = np.zeros((14, self.dims["npoin"], self.dims["nlayers"]), order="F")
        n = C.c_int64()
        self._check(lib().hnumo_cov_sums(self.h, _dp(out), out.size, C.byref(n)))
        return out, n.value

    def cov_set_sums(self, sums, nsamples: int):
        """Restore sums (14, npoin, nlayers) and a sample count, e.g. of a run being restarted."""
        a = np.array(sums, dtype=np.float64, order="F")
        size = 14 * self.dims["npoin"] * self.dims["nlayers"]
        self._check(lib().hnumo_cov_set_sums(self.h, _dp(a, size, "sums"), a.size, int(nsamples)))

    def cov_fields(self):
        """(16, npoin, nlayers) in the order of covariance.FIELD_NAMES, of the samples so far."""
        out = np.zeros((16, self.dims["npoin"], self.dims["nlayers"]), order="F")
        self._check(lib().hnumo_cov_fields(self.h, _dp(out), out.size))
        return out

    def cov_integrals(self):
        """(3, nlayers): the integrals of hbar*(0.5*(Ruu+Rvv)), dvar and hbar*ens over the owned elements."""
        out = np.zeros((3, self.dims["nlayers"]), order="F")
        self._check(lib().hnumo_cov_integrals(self.h, _dp(out), out.size))
        return out

    def cov_end(self):
        self._check(lib().hnumo_cov_end(self.h))

    # ---- energy budget of the device state (hnumo_energy_*; mirror: hnumo/energy.py)
    def energy_begin(self, zref=None, every: int = 0, series: int = 0):
        """Allocate and zero the running sums (again: reset).  zref (npoin, nlayers), or None: 0.  every =
        k >= 1: the engine samples itself after every k-th successful step; series: samples the series of
        3*nlayers + 2 integrals can hold (0: none)."""
        npoin, L = self.dims["npoin"], self.dims["nlayers"]
        zp = None
        if zref is not None:
            z = np.array(zref, dtype=np.float64, order="F")
            if z.shape != (npoin, L):
                raise ValueError(f"zref: shape {z.shape}, expected (npoin, nlayers) = ({npoin}, {L})")
            zp = z.ctypes.data_as(C.POINTER(C.c_double))
        self._check(lib().hnumo_energy_begin(self.h, zp, int(every), int(series)))

    def energy_sample(self):
        """One sample of the state and the wind on the device; nothing is copied back."""
        self._check(lib().hnumo_energy_sample(self.h))

    def energy_series(self, clear: bool = False):
        """(3*nlayers + 2, count) = KE_1..L, APE_1..L, V_1..L, W, D per sample; clear empties the series."""
        return self._series(lib().hnumo_energy_series, (3 * self.dims["nlayers"] + 2,), clear=clear)

    def _energy_out(self):
        return (np.zeros((2, self.dims["npoin_q"]), order="F"), np.zeros((self.dims["npoin"], self.dims["nlayers"]), order="F"))

    def energy_sums(self):
        """(quad (2, npoin_q) = S_W, S_D; nodal (npoin, nlayers) = S_V; the sample count)."""
        quad, nodal = self._energy_out()
        n = C.c_int64()
        self._check(lib().hnumo_energy_sums(self.h, _dp(quad), quad.size, _dp(nodal), nodal.size, C.byref(n)))
        return quad, nodal, n.value

    def energy_set_sums(self, quad, nodal, nsamples: int):
        """Restore the sums and a sample count, e.g. of a run being restarted."""
        a, b = np.array(quad, dtype=np.float64, order="F"), np.array(nodal, dtype=np.float64, order="F")
        d = self.dims
        self._check(lib().hnumo_energy_set_sums(self.h, _dp(a, 2 * d["npoin_q"], "quad"), a.size,
                                                _dp(b, d["npoin"] * d["nlayers"], "nodal"), b.size, int(nsamples)))

    def energy_means(self):
        """(quad (2, npoin_q) = S_W/N, S_D/N; nodal (npoin, nlayers) = S_V/N): the maps of mean wind power
        input, drag and dissipation."""
        quad, nodal = self._energy_out()
        self._check(lib().hnumo_energy_means(self.h, _dp(quad), quad.size, _dp(nodal), nodal.size))
        return quad, nodal

    def energy_end(self):
        self._check(lib().hnumo_energy_end(self.h))

    # ---- region sets on the device state (hnumo_regions_*; mirror and helpers: hnumo/regions.py)
    def regions_create(self, labels, nregions: int, rows: int = abi.REGION_FLOW, coriolis_df=None, every: int = 0,
                       series: int = 0) -> int:
        """A set from labels (nelem_owned) in 0..nregions (0: in no region); rows: abi.REGION_FLOW, REGION_VORT or
        their sum; coriolis_df (npoin), or None: f = 0.  every = k >= 1: the engine samples after every k-th
        successful step; series: samples the series can hold.  Returns its id."""
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        fp = None
        if coriolis_df is not None:
            f = np.ascontiguousarray(np.asarray(coriolis_df, dtype=np.float64).reshape(-1))
            if f.size != self.dims["npoin"]:
                raise ValueError(f"coriolis_df: {f.size} elements, expected {self.dims['npoin']}")
            fp = f.ctypes.data_as(C.POINTER(C.c_double))
        sid = C.c_int32(-1)
        self._check(lib().hnumo_regions_create(self.h, lab.ctypes.data_as(C.POINTER(C.c_int32)), lab.size, int(nregions), int(rows),
                                               fp, int(every), int(series), C.byref(sid)))
        self._sets("region")[sid.value] = (int(nregions), abi.region_rows(self.dims["nlayers"], int(rows)))
        return sid.value

    def regions_sample(self, sid: int):
        """Append one sample to the set's series on the device; nothing is copied back."""
        self._check(lib().hnumo_regions_sample(self.h, int(sid)))

    def regions_series(self, sid: int, clear: bool = False):
        """(V, nregions, count): the recorded samples; clear empties the series afterwards."""
        R, V = self._set_sizes("region", sid)
        return self._series(lib().hnumo_regions_series, (V, R), int(sid), clear=clear)

    def regions_area(self, sid: int):
        """(nregions,): the sum of the nodal jac per region."""
        out = np.zeros(self._set_sizes("region", sid)[0])
        self._check(lib().hnumo_regions_area(self.h, int(sid), _dp(out), out.size))
        return out

    def regions_destroy(self, sid: int):
        self._check(lib().hnumo_regions_destroy(self.h, int(sid)))
        self._sets("region").pop(sid, None)

    # ---- sample sets on the device state (hnumo_sample_*; mirror and helpers: hnumo/sample.py)
    def _sample_nval(self, source: int) -> int:
        L = self.dims["nlayers"]
        if source == SAMPLE_COV:
            return 16 * L
        return 4 * L if source == SAMPLE_VORT else 5 * L if source == SAMPLE_STATS else 5 * L + 4

    def sample_create(self, coord, xgl, xy, source: int = 0) -> int:
        """A set from physical points xy (2, M), located in the owned elements from coord
        (2 or 3, npoin) and the LGL nodes xgl; source: SAMPLE_STATE or SAMPLE_STATS.  Returns its id."""
        coord, xgl, xy = self._coord_arg(coord), self._sample_xgl(xgl), self._xy_arg(xy)
        sid = C.c_int32(-1)
        dp = C.POINTER(C.c_double)
        self._check(lib().hnumo_sample_create(self.h, coord.ctypes.data_as(dp), coord.shape[0], xgl.ctypes.data_as(dp),
                                              xy.ctypes.data_as(dp), xy.shape[1], int(source), C.byref(sid)))
        self._sets("sample")[sid.value] = (xy.shape[1], self._sample_nval(source))
        return sid.value

    def sample_create_ref(self, xgl, elem, xi_eta, source: int = 0) -> int:
        """A set from given locations: elem (M) 1-based local elements (0: not on this rank) and
        xi_eta (2, M) in [-1,1].  Returns its id."""
        xgl = self._sample_xgl(xgl)
        elem = np.ascontiguousarray(elem, dtype=np.int32).reshape(-1)
        xe = np.asfortranarray(xi_eta, dtype=np.float64)
        if xe.ndim != 2 or xe.shape != (2, elem.size):
            raise ValueError(f"xi_eta: shape {xe.shape}, expected (2, {elem.size})")
        sid = C.c_int32(-1)
        dp = C.POINTER(C.c_double)
        self._check(lib().hnumo_sample_create_ref(self.h, xgl.ctypes.data_as(dp), elem.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  xe.ctypes.data_as(dp), elem.size, int(source), C.byref(sid)))
        self._sets("sample")[sid.value] = (elem.size, self._sample_nval(source))
        return sid.value

    def _sample_xgl(self, xgl):
        xgl = np.ascontiguousarray(xgl, dtype=np.float64).reshape(-1)
        if xgl.size != self.dims["ngl"]:
            raise ValueError(f"xgl: {xgl.size} nodes, expected ngl = {self.dims['ngl']}")
        return xgl

    def sample_plan(self, sid: int):
        """(elem (M) int32, xi_eta (2, M)) of the set."""
        return self._plan(lib().hnumo_sample_plan, sid, self._set_sizes("sample", sid)[0])

    def sample(self, sid: int):
        """(V, M): the set sampled on the device now (no sync)."""
        M, V = self._set_sizes("sample", sid)
        out = np.zeros((V, M), order="F")
        self._check(lib().hnumo_sample(self.h, int(sid), _dp(out), out.size))
        return out

    def sample_series_begin(self, sid: int, every: int = 0, capacity: int = 0):
        """(Re)allocate the set's series of `capacity` samples on the device.  every = k >= 1: the
        engine records after every k-th successful step; every = 0: sample_record() does."""
        self._check(lib().hnumo_sample_series_begin(self.h, int(sid), int(every), int(capacity)))

    def sample_record(self, sid: int):
        """Append one sample to the set's series on the device; nothing is copied back."""
        self._check(lib().hnumo_sample_record(self.h, int(sid)))

    def sample_series(self, sid: int, clear: bool = False):
        """(V, M, count): the recorded samples; clear empties the series afterwards."""
        M, V = self._set_sizes("sample", sid)
        return self._series(lib().hnumo_sample_series, (V, M), int(sid), clear=clear)

    def sample_destroy(self, sid: int):
        self._check(lib().hnumo_sample_destroy(self.h, int(sid)))
        self._sets("sample").pop(sid, None)

    # ---- float sets on the device state (hnumo_floats_*; mirror and helpers: hnumo/floats.py)
    def _floats_seeds(self, xy, layer):
        xy = self._xy_arg(xy)
        layer = np.ascontiguousarray(np.broadcast_to(np.asarray(layer, dtype=np.int32), (xy.shape[1],)))
        return xy, layer

    def floats_create(self, coord, xgl, xy, layer) -> int:
        """A float set seeded at xy (2, M) in the layers `layer` (M, or one for all; 1-based), located in
        the owned elements from coord (2 or 3, npoin) and the LGL nodes xgl.  Returns its id."""
        coord, xgl = self._coord_arg(coord), self._sample_xgl(xgl)
        xy, layer = self._floats_seeds(xy, layer)
        fid = C.c_int32(-1)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        self._check(lib().hnumo_floats_create(self.h, coord.ctypes.data_as(dp), coord.shape[0], xgl.ctypes.data_as(dp),
                                              xy.ctypes.data_as(dp), layer.ctypes.data_as(ip), xy.shape[1], C.byref(fid)))
        self._sets("float")[fid.value] = xy.shape[1]
        return fid.value

    def floats_get(self, fid: int) -> dict:
        """x, y, u, v (M, float64), elem, status (M, int32) in input order; u, v = the stored velocity."""
        M = self._set_sizes("float", fid)
        f = {k: np.zeros(M) for k in ("x", "y", "u", "v")}
        i = {k: np.zeros(M, dtype=np.int32) for k in ("elem", "status")}
        ip = C.POINTER(C.c_int32)
        self._check(lib().hnumo_floats_get(self.h, int(fid), _dp(f["x"]), _dp(f["y"]), _dp(f["u"]), _dp(f["v"]),
                                           i["elem"].ctypes.data_as(ip), i["status"].ctypes.data_as(ip), M))
        return {**f, **i}

    def floats_plan(self, fid: int):
        """(elem (M) int32, xi_eta (2, M)): the floats' cached locations in input order."""
        return self._plan(lib().hnumo_floats_plan, fid, self._set_sizes("float", fid))

    def floats_set(self, fid: int, xy, layer):
        """Re-seed and relocate the set's M floats."""
        M = self._set_sizes("float", fid)
        xy, layer = self._floats_seeds(xy, layer)
        self._check(lib().hnumo_floats_set(self.h, int(fid), xy.ctypes.data_as(C.POINTER(C.c_double)),
                                           layer.ctypes.data_as(C.POINTER(C.c_int32)), xy.shape[1]))

    def floats_advance(self, fid: int, dt: float):
        """One advance by dt on the state on the device now; nothing is copied back."""
        self._check(lib().hnumo_floats_advance(self.h, int(fid), float(dt)))

    def floats_begin(self, fid: int, every: int = 1, record_every: int = 0, capacity: int = 0):
        """every = 1: the engine advances the set by dt after every successful step.  A record is
        appended to a series of `capacity` records after every record_every-th advance."""
        self._check(lib().hnumo_floats_begin(self.h, int(fid), int(every), int(record_every), int(capacity)))

    def floats_record(self, fid: int):
        """Append one record to the set's series on the device; nothing is copied back."""
        self._check(lib().hnumo_floats_record(self.h, int(fid)))

    def floats_series(self, fid: int, clear: bool = False):
        """(5 + S, M, count) = x, y, u, v, elem and the set's S sensor rows per record; clear empties the
        series afterwards."""
        M = self._set_sizes("float", fid)
        return self._series(lib().hnumo_floats_series, (5 + self.floats_sense_info(fid)[0], M), int(fid), clear=clear)

    def floats_sensors(self, fid: int, mask: int):
        """The set's sensor mask (abi.FLOAT_SENSE_STATE + abi.FLOAT_SENSE_VORT; 0: none): S rows of the float's
        own layer behind the 5 of every record.  Sensors first, then floats_begin."""
        self._check(lib().hnumo_floats_sensors(self.h, int(fid), int(mask)))

    def floats_sense(self, fid: int):
        """(S, M): the set's sensors on the state on the device now, in input order."""
        M = self._set_sizes("float", fid)
        out = np.zeros((self.floats_sense_info(fid)[0], M), order="F")
        buf = out if out.size else np.zeros(1)
        self._check(lib().hnumo_floats_sense(self.h, int(fid), _dp(buf), out.size))
        return out

    def floats_sense_info(self, fid: int):
        """(S, K): the sensor rows of the set and the element slots of the sensor kernel's arena."""
        S, K = C.c_int32(), C.c_int32()
        self._check(lib().hnumo_floats_sense_info(self.h, int(fid), C.byref(S), C.byref(K)))
        return S.value, K.value

    def floats_destroy(self, fid: int):
        self._check(lib().hnumo_floats_destroy(self.h, int(fid)))
        self._sets("float").pop(fid, None)

    def floats_migrate(self, fid: int, on: bool = True, coord_scale: float = 0.0):
        """The set hands floats that reach a processor face to the rank across it (processor-face ranks)."""
        self._check(lib().hnumo_floats_migrate(self.h, int(fid), int(bool(on)), float(coord_scale)))

    def floats_release(self, fid: int, idx):
        """The floats at the 0-based input positions idx that are ACTIVE on this rank become LEFT."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        self._check(lib().hnumo_floats_release(self.h, int(fid), idx.ctypes.data_as(C.POINTER(C.c_int32)), idx.size))

    def floats_outbox(self, fid: int):
        """(d (7, n), i (6, n)): the flight records waiting on this rank, sorted by gid; d = x, y, wx, wy, dt,
        px, py and i = gid, layer, stage, hops, destination rank, pos.  The outbox is empty afterwards."""
        M = self._set_sizes("float", fid)
        d, i = np.zeros((7, M)), np.zeros((6, M), dtype=np.int32)
        n = C.c_int64()
        self._check(lib().hnumo_floats_outbox(self.h, int(fid), d.ctypes.data_as(C.POINTER(C.c_double)),
                                              i.ctypes.data_as(C.POINTER(C.c_int32)), M, C.byref(n)))
        return d[:, :n.value].copy(), i[:, :n.value].copy()

    def floats_deliver(self, fid: int, src_rank: int, d, i):
        """Runs the arrivals of the flight records (d (7, n), i (6, n)) that rank src_rank sent."""
        d, i = np.ascontiguousarray(d, dtype=np.float64), np.ascontiguousarray(i, dtype=np.int32)
        n = d.shape[1]
        if d.ndim != 2 or d.shape[0] != 7 or i.shape != (6, d.shape[1]):
            raise ValueError(f"deliver: d {d.shape}, i {i.shape}, expected (7, n) and (6, n)")
        self._check(lib().hnumo_floats_deliver(self.h, int(fid), int(src_rank), d.ctypes.data_as(C.POINTER(C.c_double)),
                                               i.ctypes.data_as(C.POINTER(C.c_int32)), n, n))

    def floats_settle(self, fid: int):
        """Takes the record that an advance of a migrating set deferred."""
        self._check(lib().hnumo_floats_settle(self.h, int(fid)))

    # ---- time-dependent wind stress (hnumo_wind_*; mirror and schedules: hnumo/wind.py)
    def wind_begin(self, patterns):
        """patterns (2, npoin_q, M), 1 <= M <= 4, over every local element.  The wind is unchanged until
        wind_set or a scheduled step; again: replaces the patterns and clears the schedule."""
        p = np.asfortranarray(patterns, dtype=np.float64)
        if p.ndim == 2:
            p = np.asfortranarray(p[:, :, None])
        if p.ndim != 3 or p.shape[:2] != (2, self.dims["npoin_q"]):
            raise ValueError(f"patterns: shape {p.shape}, expected (2, {self.dims['npoin_q']}, M)")
        self._check(lib().hnumo_wind_begin(self.h, p.ctypes.data_as(C.POINTER(C.c_double)), p.size, p.shape[2]))

    def wind_set(self, coef):
        """tau_wind = coef[0]*T_0 + coef[1]*T_1 + ... now, for every later step (hnumo.wind.blend)."""
        c = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
        self._check(lib().hnumo_wind_set(self.h, c.ctypes.data_as(C.POINTER(C.c_double)), c.size))

    def wind_schedule(self, coef, first: int = 0, mode=0):
        """coef (M, nrows), copied to the device once: the k-th successful step from now uses row first + k,
        held at the last row (mode "hold") or taken modulo nrows ("repeat").  No rows: clears the schedule."""
        from .wind import _mode
        t = np.asfortranarray(coef, dtype=np.float64)
        if t.ndim != 2:
            raise ValueError(f"coef: shape {t.shape}, expected (M, nrows)")
        self._check(lib().hnumo_wind_schedule(self.h, t.ctypes.data_as(C.POINTER(C.c_double)), t.shape[0], t.shape[1],
                                              int(first), _mode(mode)))

    def wind_get(self):
        """(tau_wind (2, npoin_q) on the device now, the row the next step will use or -1)."""
        tau = np.zeros((2, self.dims["npoin_q"]), order="F")
        r = C.c_int32(-2)
        self._check(lib().hnumo_wind_get(self.h, _dp(tau), tau.size, C.byref(r)))
        return tau, r.value

    def wind_end(self):
        """The create-time wind again, bit for bit; frees the patterns and the schedule."""
        self._check(lib().hnumo_wind_end(self.h))

    def bench_steps(self, nsteps: int):
        t = C.c_double()
        k = C.c_double()
        n = C.c_int64()
        self._check(lib().hnumo_bench_steps(self.h, nsteps, C.byref(t), C.byref(k), C.byref(n)))
        return t.value, k.value, n.value

    def time_stage_kernel(self, nsubcycles: int = 2) -> float:
        """Average btp_stage_kernel duration (ms), HIP events on the engine stream."""
        k = C.c_double()
        self._check(lib().hnumo_time_stage_kernel(self.h, nsubcycles, C.byref(k)))
        return k.value

    def stage_profile(self):
        n = self.dims["nelem"] * 32
        out = np.zeros(n, dtype=np.uint64)
        self._check(lib().hnumo_debug_stage_profile(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n))
        return out.reshape(-1, 32)

    def step_breakdown(self, nsteps: int = 2) -> dict:
        """Microseconds per step of every kernel family of the step, in launch order
        (hnumo_step_breakdown: direct launches with an event after each; the state advances)."""
        names = C.create_string_buffer(4096)
        us = (C.c_double * 64)()
        n = C.c_int()
        self._check(lib().hnumo_step_breakdown(self.h, nsteps, names, len(names), us, 64, C.byref(n)))
        keys = names.value.decode().split("\n") if n.value else []
        return {k: us[i] for i, k in enumerate(keys)}

    @staticmethod
    def stream_copy_bw(device: int = 0, nbytes: int = 1 << 30, reps: int = 10) -> tuple:
        """(GB/s, variant) of the fastest 16-byte stream copy between two buffers of nbytes, reps
        launches back to back (read + write counted; hnumo_stream_copy_bw)."""
        out = (C.c_double * 2)()
        rc = lib().hnumo_stream_copy_bw(device, nbytes, reps, out)
        if rc:
            raise EngineError(rc, "stream copy measurement failed")
        return out[0], out[1]

    @staticmethod
    def rccl_unique_id() -> bytes:
        buf = (C.c_ubyte * 128)()
        rc = lib().hnumo_rccl_unique_id(buf)
        if rc:
            raise EngineError(rc, "ncclGetUniqueId failed")
        return bytes(buf)

    def _destroy(self):
        if getattr(self, "h", None) is not None and self.h.value:
            lib().hnumo_engine_destroy(self.h)
            self.h = C.c_void_p()

    def close(self):
        self._destroy()

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass


def local_group(engines):
    """Join the engines of one process (ranks 0..n-1, same device) into a local exchange group."""
    arr = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
    rc = lib().hnumo_local_group(arr, len(engines))
    if rc:
        raise EngineError(rc, "hnumo_local_group failed (ranks must be 0..n-1 on one device)")
    for e in engines:
        e._group = arr


def group_ti_rk_bcl(engines, states):
    """One baroclinic step of every engine of a local group; states[i] = (q, qb, qp) arrays."""
    n = len(engines)
    if len(states) != n:
        raise ValueError("one (q, qb, qp) state per engine")
    arr = engines[0]._group
    ptrs = [e._state_ptrs(*states[i]) for i, e in enumerate(engines)]
    mk = lambda j: (C.POINTER(C.c_double) * n)(*[ptrs[i][j] for i in range(n)])
    rc = lib().hnumo_group_ti_rk_bcl(arr, n, mk(0), mk(1), mk(2))
    if rc:
        msgs = [lib().hnumo_last_error(e.h).decode() for e in engines]
        raise EngineError(rc, "; ".join(m for m in msgs if m))


def _group_check(engines, rc):
    if rc:
        msgs = [lib().hnumo_last_error(e.h).decode() for e in engines]
        raise EngineError(rc, "; ".join(m for m in msgs if m))


def group_floats_migrate(engines, fid: int, on: bool = True, coord_scale: float = 0.0):
    """hnumo_floats_migrate on every engine of a local group; a seed ACTIVE on several ranks stays on the lowest."""
    _group_check(engines, lib().hnumo_group_floats_migrate(engines[0]._group, len(engines), int(fid), int(bool(on)), float(coord_scale)))


def group_floats_advance(engines, fid: int, dt: float):
    """One advance by dt of the migrating set fid on every engine of a local group, and its arrivals."""
    _group_check(engines, lib().hnumo_group_floats_advance(engines[0]._group, len(engines), int(fid), float(dt)))
