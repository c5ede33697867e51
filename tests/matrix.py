"""The parity matrix: one list of named cells shared by the CPU and the GPU tests (a plain helper
module).

The kernels are templates on the order N with per-N work splits and LDS budgets, carry MAXL-sized
register arrays guarded by the layer count, and branch on the viscosity method, the wall codes,
the drag law, the shear solve and the mesh kind.  A cell crosses one level of each of these
factors on the smallest mesh that still has every kind of element (4x4 for N <= 4; 3x3 for
N >= 5, the smallest with an element all of whose neighbours are distinct interior elements) and
starts, but for a few controls at rest, from a state that moves (tests/states.py).

CELLS is chosen so that every pair of levels of (N x each other factor) and of (layer family x
each other factor) occurs, and so that the N = 7 rows and the single-layer rows together see
every level of every other factor; tests/test_states_cpu.py asserts both, so that an edit cannot
quietly thin the list.

VARIANTS names the device code that an engine of 2,048 owned elements or more switches to (engine.hip,
read_knobs): the LEAN arenas of the per-stage barotropic kernel (N = 4 only) and the large-mesh layer
mass / consistency kernels (every N).  Neither depends on the mesh size in anything but that choice,
so the experiment knobs force them onto the cells' 16 or 9 elements, and the cells' own oracle
results judge them.  The N = 4 rows -- all that the LEAN arenas can see -- must by themselves hold
every level of every other factor (test_states_cpu.py again).
"""
import math

# factor -> levels.  A cell is (N, family, visc, walls, botfr, shear, mesh, state).
FACTORS = ("N", "family", "visc", "walls", "botfr", "shear", "mesh", "state")
LEVELS = {
    "N": (2, 3, 4, 5, 7),
    # lake: bathymetry, L = 1, 2, 3; bump: flat bottom, L = 2; dg3: wind, f, beta, L = 3
    "family": ("lake1", "lake2", "lake3", "bump2", "dg3"),
    "visc": (0, 1, 3),                          # method_visc
    "walls": ("free", "noslip", "mixed"),
    "botfr": (0, 1, 2),
    "shear": (0, 1),                            # ad_mlswe = 0; > 0 with shear_corrector = 1
    "mesh": ("brick", "warp"),
    "state": ("rest", "moving"),
}
FAMILY = {  # base configuration, layers, viscosity when method_visc != 0, max_shear_dz of the shear level
    "lake1": ("lake10", 1, 25.0, 10.0), "lake2": ("lake10", 2, 25.0, 10.0), "lake3": ("lake10", 3, 25.0, 10.0),
    "bump2": ("bump10", 2, 25.0, 10.0), "dg3": ("dg25L3", 3, 50.0, 50.0),
}
WALLS = {"free": dict(x_boundary=(4, 4), y_boundary=(4, 4)), "noslip": dict(x_boundary=(2, 2), y_boundary=(2, 2)),
         "mixed": dict(x_boundary=(2, 4), y_boundary=(4, 4))}
CD = {0: 0.0, 1: 1.0e-7, 2: 1.0e-3}             # as the branch variants of tests/test_engine_gpu.py

# a 5 x 5 Latin-square design over (N, family) with the other factors cycled along both axes, and
# five more rows that break the design's own correlation between the walls and the drag law
#  N family visc walls botfr shear mesh state
_ROWS = """
2 lake1 0 free   0 0 brick rest
2 lake2 1 mixed  1 0 brick moving
2 lake3 3 noslip 2 0 brick moving
2 bump2 0 free   0 1 warp  moving
2 dg3   1 mixed  1 1 brick moving
3 lake1 1 noslip 2 1 warp  moving
3 lake2 3 free   0 1 brick moving
3 lake3 0 mixed  1 0 brick moving
3 bump2 1 noslip 2 0 brick rest
3 dg3   3 free   0 0 brick moving
4 lake1 3 mixed  1 0 brick moving
4 lake2 0 noslip 2 0 warp  rest
4 lake3 1 free   0 1 brick moving
4 bump2 3 mixed  1 1 brick moving
4 dg3   0 noslip 2 0 warp  moving
5 lake1 0 free   0 1 warp  moving
5 lake2 1 mixed  1 0 brick moving
5 lake3 3 noslip 2 0 warp  moving
5 bump2 0 free   0 0 warp  moving
5 dg3   1 mixed  1 1 brick rest
7 lake1 1 noslip 2 0 brick moving
7 lake2 3 free   0 1 brick moving
7 lake3 0 mixed  1 1 brick rest
7 bump2 1 noslip 2 0 brick moving
7 dg3   3 free   0 0 warp  moving
2 lake1 3 noslip 1 1 brick moving
3 dg3   0 mixed  2 1 brick moving
4 lake1 1 free   2 1 warp  moving
5 bump2 3 noslip 0 1 brick moving
7 lake2 1 free   1 0 warp  moving
"""


def _cells():
    out = []
    for line in _ROWS.strip().splitlines():
        v = line.split()
        c = dict(N=int(v[0]), family=v[1], visc=int(v[2]), walls=v[3], botfr=int(v[4]), shear=int(v[5]), mesh=v[6],
                 state=v[7])
        c["nsteps"] = 1 if c["N"] == 7 else 2
        c["name"] = "N{N}-{family}-v{visc}-{walls}-b{botfr}-s{shear}-{mesh}-{state}".format(**c)
        out.append(c)
    return out


CELLS = _cells()
BY_NAME = {c["name"]: c for c in CELLS}
# the processor-face halo on a moving state (brick cells without the shear solve): N = 7 with L = 1, N = 2,
# L = 1 at N = 4, three layers at N = 3, N = 5
HALO_CELLS = ("N7-lake1-v1-noslip-b2-s0-brick-moving", "N2-lake2-v1-mixed-b1-s0-brick-moving",
              "N4-lake1-v3-mixed-b1-s0-brick-moving", "N3-lake3-v0-mixed-b1-s0-brick-moving",
              "N5-lake2-v1-mixed-b1-s0-brick-moving")


# kernel variant -> (the environment that forces it at engine creation, the orders N it applies to)
_LARGE = dict(HNUMO_EXPERIMENTS="1", HNUMO_PERSISTENT="0", HNUMO_STAGE_NB="5", HNUMO_BCL_BIG="1")
VARIANTS = {
    # what a mesh of >= 2,048 owned elements runs: the 5-per-CU LEAN arena and the large-mesh mass / cons kernels
    "large": (_LARGE, LEVELS["N"]),
    # the 4-per-CU LEAN arena; the arena knob has no effect but at N = 4, so elsewhere this would repeat "large"
    "large-nb4": (dict(_LARGE, HNUMO_STAGE_NB="4"), (4,)),
}


def variant_cells(variant):
    """The cells a kernel variant applies to."""
    return [c for c in CELLS if c["N"] in VARIANTS[variant][1]]


def variant_env(variant):
    return dict(VARIANTS[variant][0])


def variant_overrides(variant):
    """What Engine.overrides lists under a variant: the honoured settings in the order the engine reads them
    (HNUMO_EXPERIMENTS is the gate, not a setting)."""
    env = VARIANTS[variant][0]
    return [k + "=" + env[k] for k in ("HNUMO_STAGE_NB", "HNUMO_BCL_BIG", "HNUMO_PERSISTENT")]


def variant_kernels(variant, N):
    """Engine.kernel_variants of an order-N engine under a variant: the arena only where N = 4 has one."""
    env = VARIANTS[variant][0]
    return dict(stage_arena=int(env["HNUMO_STAGE_NB"]) if N == 4 else 0, bcl_big=env["HNUMO_BCL_BIG"] == "1")


def cell_config(cell):
    """(configuration name, overrides) of a cell.  The time steps are the base configuration's,
    scaled by the element size and, above N = 4, by (4/N)^2 -- as bump16 and dg25N7L3 scale theirs
    (hnumo/case.py) -- and then quartered: the base steps sit at the stability limit of a state at
    rest on a brick, and a moving state, on a warped mesh above all, goes non-finite or negative at
    them within two steps.  The number of barotropic sub-steps per step stays the base
    configuration's."""
    from hnumo.case import CONFIGS
    base, L, visc, shear_dz = FAMILY[cell["family"]]
    b = CONFIGS[base]
    n = 4 if cell["N"] <= 4 else 3
    s = 0.25 * (b["nelx"] / n) * min(1.0, (4.0 / cell["N"]) ** 2)
    nbtp = math.ceil(b["dt"] / b["dt_btp"])
    dt = b["dt"] * s
    ov = dict(nelx=n, nely=n, nop=cell["N"], nlayers=L, dt=dt, dt_btp=dt / (nbtp - 0.5),
              method_visc=cell["visc"], visc=visc if cell["visc"] else 0.0, botfr=cell["botfr"], cd=CD[cell["botfr"]])
    ov.update(WALLS[cell["walls"]])
    if cell["shear"]:
        ov.update(ad_mlswe=1.0e-2, max_shear_dz=shear_dz, shear_corrector=1)
    if cell["mesh"] == "warp":
        ov["mesh"] = ("warp", 0.15, True)
    return base, ov


def cell_case(cell, case_factory=None, dense=True):
    """The Case of a cell carrying the cell's state."""
    from hnumo.case import build_case, make_config
    import states
    name, ov = cell_config(cell)
    case = case_factory(name, **ov) if case_factory else build_case(make_config(name, **ov), dense=dense)
    return states.moving_case(case) if cell["state"] == "moving" else case


def missing_pairs(cells):
    """The pairs of levels of (N x each other factor) and (family x each other factor) that no cell
    of ``cells`` has."""
    have = set()
    for c in cells:
        for a in ("N", "family"):
            for f in FACTORS:
                if f != a:
                    have.add((a, c[a], f, c[f]))
    want = {(a, la, f, lf) for a in ("N", "family") for la in LEVELS[a] for f in FACTORS if f != a for lf in LEVELS[f]}
    return sorted(want - have, key=str)


def missing_levels(cells):
    """The levels of any factor that neither an N = 7 cell nor a single-layer cell has."""
    rows = [c for c in cells if c["N"] == 7 or c["family"] == "lake1"]
    return sorted(((f, l) for f in FACTORS for l in LEVELS[f] if not any(c[f] == l for c in rows)), key=str)


def missing_levels_of(cells):
    """The levels of any factor but N that no cell of ``cells`` has."""
    return sorted(((f, l) for f in FACTORS if f != "N" for l in LEVELS[f] if not any(c[f] == l for c in cells)),
                  key=str)


def run_oracle(case, nsteps):
    """The oracle's state and parity fields after ``nsteps`` steps of ``case``'s own state."""
    import oracle as O
    from hnumo import bundle as B
    o = O.Oracle(case)
    st = o.state()
    for _ in range(nsteps):
        o.ti_rk_bcl(*st)
    return st, {f: o.field(f) for f, _ in B.FIELDS}
