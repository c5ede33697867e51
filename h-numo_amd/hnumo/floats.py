"""Lagrangian floats: drifters that live in a layer and move with its velocity -- the one standard
online product a run cannot rebuild from its mlswe#### snapshots, because a trajectory needs the
velocity at the float's own position at every step.

    HostFloats          the Python statement of the definitions, fed with synced states on the host
    DeviceFloats        the same floats in the engine, which advances them where the state lives
                        (kernels_float.hip through hnumo_floats_*): no sync, a series kept on the device
    seed_grid           nx x ny seeds inside the owned elements' bounding box
    seed_ring           n seeds on a circle
    write_trajectories  one .npz: the series, the layers, the status

Definitions (normative; include/hnumo_engine.h).  All arithmetic is IEEE double,
no FMA.  A float carries (x, y), a layer k (1-based, fixed), a stored velocity w = (wx, wy), a cached
location (elem, xi, eta) and a status: ACTIVE, LEFT (it reached a processor face or a ghost element;
also "not on this rank at creation"), LOST.

vel(e, xi, eta): nodal U(I) = q(2,I,k)/q(1,I,k), V(I) = q(3,I,k)/q(1,I,k), I = e*P + j*ngl + i, under
    hnumo.sample's interpolant: sum_j Ly[j] * (sum_i Lx[i] * U), left to right from the first product.
locate(p, e): (1) invert e's bilinear map at p -- Newton from the element centre, at most 32
    iterations, the sample sets' loop; no finite solution: LOST; (2) max(|xi|, |eta|) <= 1 + tol_e:
    clamp to [-1,1], accept; (3) else the side with the larger excess (|xi| - 1 against |eta| - 1, a
    tie goes to xi; the sign selects the face): an owned neighbour -> go on there at (1); a physical
    boundary -> that coordinate = +-1 exactly and p = e's map at the new (xi, eta): the float slides
    along the wall, (1) again in e; a processor face or a ghost neighbour -> LEFT; (4) a fifth pass
    through (3) -> LOST.
advance(dt): Heun with the field of the new time level (w is from the previous one)
    if fresh: w = vel(elem, xi, eta); fresh = 0
    p* = (x + dt*wx, y + dt*wy);  (e*, xi*, eta*, p*) = locate(p*, elem);  u* = vel(e*, xi*, eta*)
    p1 = (x + (0.5*dt)*(wx + u*x), y + (0.5*dt)*(wy + u*y));  (e1, xi1, eta1, p1) = locate(p1, e*)
    w = vel(e1, xi1, eta1);  (x, y) = p1;  (elem, xi, eta) = (e1, xi1, eta1)
    A location that ends LEFT or LOST stops the advance: (x, y) = its target, elem = 0, w = 0; a
    non-finite velocity gives LOST likewise at the target located last.  Inactive floats never change.

The two classes agree bit for bit (tests/test_floats_gpu.py), and with the C++ host statement
(tests/test_float_plan.py).

Migration (processor-face ranks, opt-in; include/hnumo_engine.h has the normative text): in a migrating set
a location that reaches (3) at a processor face puts the float in flight instead of LEFT; the rank across
the face resumes the advance at the statement where it stopped, so a float's record on the rank that
holds it is the single-rank float's, bit for bit, through any number of crossings.

    HostFloatGroup      the numpy mirror of the group protocol over one HostFloats per rank
    GroupFloats         the same set on the engines of a local group (hnumo_group_floats_*)
    merge_series        the ranks' series as one, with global element numbers

Sensors (include/hnumo_engine.h has the normative text): a set's mask SENSE_STATE + SENSE_VORT adds S = 5 + 4
rows to every record -- h, u, v, dp, elevation and zeta, delta, pv, ow of the float's own layer, each the value
a hnumo.sample set reads at the float's cached (elem, xi, eta); 0.0 for a float with elem = 0.  HostFloats
composes them of the existing mirrors (HostSampler, HostVorticity); DeviceFloats reads them from the engine
(float_sense_kernel), bit for bit the same (tests/test_float_sense_gpu.py)."""
from __future__ import annotations

import math

import numpy as np

from . import sample as _sample
from .abi import FLOAT_SENSE_STATE as SENSE_STATE, FLOAT_SENSE_VORT as SENSE_VORT, float_sense_rows as sense_rows

ACTIVE, LEFT, LOST = 0, 1, 2      # HNUMO_FLOAT_ACTIVE, HNUMO_FLOAT_LEFT, HNUMO_FLOAT_LOST
FLIGHT = 3                        # locate's answer at a processor face of a migrating set (never a float's status)
MAXROUNDS = 8                     # rounds of arrivals that settle one advance
WALL, OFF_RANK = -1, -2           # side neighbours that are no element
SIDES = ("xi=-1", "xi=+1", "eta=-1", "eta=+1")
EPS = 2.0 ** -52


def side_neighbours(case):
    """(nelem_owned, 4) int32: per owned element (0-based) and side (xi=-1, xi=+1, eta=-1, eta=+1) the
    0-based owned neighbour, WALL for a physical boundary, OFF_RANK for a processor face or a ghost
    neighbour.  From face (8, nface), imapl, imapr (3, ngl, nface) by brute force: the side is the one
    all the face's local nodes of that element lie on."""
    A, S = case.arrays, case.scalars
    ngl, ne = S["ngl"], _sample.owned_elements(case)
    face, maps = np.asarray(A["face"]), (np.asarray(A["imapl"]), np.asarray(A["imapr"]))
    nbr = np.full((ne, 4), -3, dtype=np.int32)
    for f in range(face.shape[1]):
        el, er = int(face[6, f]), int(face[7, f])
        for me, other, im in ((el, er, maps[0]), (er, el, maps[1])):
            if me < 1 or me > ne:
                continue
            i, j = im[0, :, f], im[1, :, f]
            on = [(i == 1).all(), (i == ngl).all(), (j == 1).all(), (j == ngl).all()]
            if sum(on) != 1:
                raise ValueError(f"face {f + 1}: its nodes are not one side of element {me}")
            s = on.index(True)
            if nbr[me - 1, s] != -3:
                raise ValueError(f"element {me}: two faces on side {SIDES[s]}")
            if other < 0:
                nbr[me - 1, s] = WALL
            elif other == 0 or other > ne:
                nbr[me - 1, s] = OFF_RANK
            else:
                nbr[me - 1, s] = other - 1
    if (nbr == -3).any():
        raise ValueError("an owned element has a side without a face")
    return nbr


def sense_slots(elem):
    """The slot rule of the sensor kernel for one workgroup's floats `elem` (1-based elements in slot order, <= 0:
    inactive): (slot (n) with -1 for inactive floats, the 0-based elements of the slots).  A float is a head when
    it is active and it is the first, or the float before it is inactive or in another element; a slot per head."""
    elem = np.asarray(elem).reshape(-1)
    act = elem > 0
    head = act.copy()
    head[1:] &= ~act[:-1] | (elem[1:] != elem[:-1])
    slot = np.where(act, np.cumsum(head) - 1, -1).astype(np.int32)
    return slot, (elem[head] - 1).astype(np.int32)


def _bilinear(c, xi, eta):
    """The sample sets' bilinear map of the corners c (8 floats: 4 x (x, y)) and its Jacobian."""
    w0, w1 = 0.25 * (1 - xi) * (1 - eta), 0.25 * (1 + xi) * (1 - eta)
    w2, w3 = 0.25 * (1 + xi) * (1 + eta), 0.25 * (1 - xi) * (1 + eta)
    x = [0.0, 0.0]
    J = [[0.0, 0.0], [0.0, 0.0]]
    for d in range(2):
        x[d] = w0 * c[d] + w1 * c[2 + d] + w2 * c[4 + d] + w3 * c[6 + d]
        J[d][0] = 0.25 * (-(1 - eta) * c[d] + (1 - eta) * c[2 + d] + (1 + eta) * c[4 + d] - (1 + eta) * c[6 + d])
        J[d][1] = 0.25 * (-(1 - xi) * c[d] - (1 + xi) * c[2 + d] + (1 + xi) * c[4 + d] + (1 - xi) * c[6 + d])
    return x, J


def _div(a, b):
    """IEEE division of Python floats (a zero divisor gives inf or nan, not an exception)."""
    try:
        return a / b
    except ZeroDivisionError:
        return float(np.float64(a) / np.float64(b))


def _invert(c, px, py):
    """The sample sets' Newton loop: (xi, eta), or None without a finite solution."""
    xi = eta = 0.0
    for _ in range(32):
        x, J = _bilinear(c, xi, eta)
        rx, ry = px - x[0], py - x[1]
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
        with np.errstate(all="ignore"):
            dxi, deta = _div(J[1][1] * rx - J[0][1] * ry, det), _div(J[0][0] * ry - J[1][0] * rx, det)
        if not math.isfinite(dxi) or not math.isfinite(deta):
            return None
        xi += dxi
        eta += deta
        if abs(xi) > 1e3 or abs(eta) > 1e3:
            return None
        if abs(dxi) <= 1e-16 and abs(deta) <= 1e-16:
            break
    return xi, eta


def _clamp(v):
    return min(1.0, max(-1.0, v))


class HostFloats:
    """The Python mirror: M floats of `case` (or of a rank's case of a partition) seeded at xy (2, M)
    in the layers `layer` (M, or one for all).  advance(q_df, dt) moves them on a synced state;
    get() / record() / series() read them as the engine's calls do.  A per-float Python loop."""

    needs_host_state = True

    def __init__(self, case, xy, layer, xgl=None, coord=None, coord_scale=0.0, sensors=0, coriolis=True):
        S = case.scalars
        self.sensors, self.coriolis = 0, coriolis
        self._q = None                    # the state of the last advance: what record() senses
        self.case = case
        self.ngl, self.L, self.npoin = S["ngl"], S["nlayers"], S["npoin"]
        self.P = self.ngl ** 2
        self.ne = _sample.owned_elements(case)
        self.dt = S["dt"]
        self.xgl = [float(v) for v in (_sample.case_xgl(case) if xgl is None else np.asarray(xgl).reshape(-1))]
        coord = np.asarray(case.arrays["coord"] if coord is None else coord, dtype=np.float64)
        n, P = self.ngl, self.P
        cn = np.array([0, n - 1, n * n - 1, n * (n - 1)])
        c = coord[0:2, (np.arange(self.ne) * P)[:, None] + cn[None, :]]                  # (2, ne, 4)
        self.corners = np.ascontiguousarray(c.transpose(1, 2, 0)).reshape(self.ne, 8)     # [e][corner][x|y]
        self.maxc = float(np.abs(coord[0:2, :self.ne * P]).max()) if self.ne else 0.0
        ex = np.roll(c, -1, axis=2) - c
        edge = np.sqrt(ex[0] * ex[0] + ex[1] * ex[1])                                     # (ne, 4)
        self.tol = (64.0 * EPS * self.maxc) / (0.5 * edge.min(axis=1))
        self.nbr = side_neighbours(case)
        self._c = [[float(v) for v in row] for row in self.corners]
        self._tol = [float(v) for v in self.tol]
        self._nbr = [[int(v) for v in row] for row in self.nbr]
        self._lo = c.min(axis=2) if self.ne else np.zeros((2, 0))
        self._hi = c.max(axis=2) if self.ne else np.zeros((2, 0))
        self._records = []
        self.xface = None                 # a migrating set's side table (migrate_tables), else None
        self.outbox = []                  # its flight records since it was last emptied
        self.set(xy, layer)
        if coord_scale:
            self.set_coord_scale(coord_scale)
        self.set_sensors(sensors)

    # ---- sensors
    def set_sensors(self, mask):
        """The sensor mask (hnumo_floats_sensors): refused for an unknown bit and while records of another
        width are held."""
        mask = int(mask)
        if mask < 0 or mask & ~(SENSE_STATE | SENSE_VORT):
            raise ValueError(f"sensors: the mask must be a sum of SENSE_STATE (1) and SENSE_VORT (2), got {mask}")
        if self._records and sense_rows(mask) != sense_rows(self.sensors):
            raise ValueError("sensors: the series holds records of another width (series(clear=True) first)")
        self.sensors = mask

    def sense(self, q_df):
        """(S, M): the sensor rows of every float at its cached (elem, xi, eta) on q_df (3, npoin, L)."""
        if not self.sensors:
            raise ValueError("sense: the set has no sensors")
        if q_df is None:
            raise ValueError("sense: no state yet (advance first)")
        from .vorticity import HostVorticity
        m, k = np.arange(self.M), self.layer.astype(np.int64) - 1
        rows = []
        if self.sensors & SENSE_STATE:
            hs = _sample.HostSampler(self.case, self.elem, self.xi, self.eta, _sample.STATE, xgl=self.xgl)
            full = hs.sample(q_df, np.zeros((4, self.npoin)))          # (the qb rows are not taken)
            rows += [full[5 * k + v, m] for v in range(5)]
        if self.sensors & SENSE_VORT:
            hs = _sample.HostSampler(self.case, self.elem, self.xi, self.eta, _sample.VORT, xgl=self.xgl)
            with np.errstate(all="ignore"):
                full = hs.sample_vort(HostVorticity(self.case, coriolis=self.coriolis, series=False).fields(q_df))
            rows += [full[4 * k + v, m] for v in range(4)]
        return np.asfortranarray(np.stack(rows))

    def set_coord_scale(self, scale):
        """tol_e of every later location from max|coord| = scale (0: the case's own again); seeds stay."""
        if not (scale >= 0.0 and math.isfinite(scale)):
            raise ValueError("coord_scale must be finite and >= 0")
        ex = np.roll(self.corners.reshape(self.ne, 4, 2), -1, axis=1) - self.corners.reshape(self.ne, 4, 2)
        edge = np.sqrt(ex[:, :, 0] * ex[:, :, 0] + ex[:, :, 1] * ex[:, :, 1])
        self.tol = (64.0 * EPS * (scale if scale > 0.0 else self.maxc)) / (0.5 * edge.min(axis=1))
        self._tol = [float(v) for v in self.tol]

    # ---- seeding
    def set(self, xy, layer):
        """(Re-)seed: locate xy in the owned elements as the sample sets do (the lowest accepting
        element wins; none: LEFT), w = 0, fresh = 1."""
        xy = np.asarray(xy, dtype=np.float64)
        if xy.ndim != 2 or xy.shape[0] != 2 or xy.shape[1] < 1:
            raise ValueError(f"xy: shape {xy.shape}, expected (2, M) with M >= 1")
        M = xy.shape[1]
        if hasattr(self, "M") and M != self.M:
            raise ValueError(f"set: M must be the set's {self.M}")
        layer = np.broadcast_to(np.asarray(layer, dtype=np.int32), (M,)).copy()
        if (layer < 1).any() or (layer > self.L).any():
            raise ValueError(f"layer must lie in 1..{self.L}")
        self.M = M
        self.x, self.y = xy[0].copy(), xy[1].copy()
        self.wx, self.wy, self.xi, self.eta = (np.zeros(M) for _ in range(4))
        self.elem, self.status = np.zeros(M, dtype=np.int32), np.full(M, LEFT, dtype=np.int32)
        self.layer, self.fresh = layer, np.ones(M, dtype=np.int32)
        size = (self._hi - self._lo).sum(axis=0) if self.ne else np.zeros(0)
        pad = 1e-6 * size                                   # >> tol_e in x, y: only a quick reject
        for m in range(M):
            px, py = float(xy[0, m]), float(xy[1, m])
            if not (math.isfinite(px) and math.isfinite(py)):
                continue
            cand = np.nonzero((px >= self._lo[0] - pad) & (px <= self._hi[0] + pad) &
                              (py >= self._lo[1] - pad) & (py <= self._hi[1] + pad))[0]
            for e in cand:
                r = _invert(self._c[e], px, py)
                if r is None or not max(abs(r[0]), abs(r[1])) <= 1.0 + self._tol[e]:
                    continue
                self.elem[m], self.status[m] = e + 1, ACTIVE
                self.xi[m], self.eta[m] = _clamp(r[0]), _clamp(r[1])
                break
        # per float the 1-based elements its locations have gone through (tests read it)
        self.visited = [{int(e)} if e else set() for e in self.elem]

    # ---- the three definitions
    def vel(self, q, k, e, xi, eta):
        """(u, v) of layer k (0-based) at (e, xi, eta), e 0-based, on q_df (3, npoin, L)."""
        ngl, g = self.ngl, self.xgl
        lx, ly = [], []
        for i in range(ngl):
            wx = wy = 1.0
            for m in range(ngl):
                if m != i:
                    wx = wx * ((xi - g[m]) / (g[i] - g[m]))
                    wy = wy * ((eta - g[m]) / (g[i] - g[m]))
            lx.append(wx)
            ly.append(wy)
        blk = q[:, e * self.P:(e + 1) * self.P, k]
        with np.errstate(all="ignore"):
            U, V = (blk[1] / blk[0]).tolist(), (blk[2] / blk[0]).tolist()
        u = v = 0.0
        for j in range(ngl):
            ru, rv = lx[0] * U[j * ngl], lx[0] * V[j * ngl]
            for i in range(1, ngl):
                ru = ru + lx[i] * U[j * ngl + i]
                rv = rv + lx[i] * V[j * ngl + i]
            u = ly[0] * ru if j == 0 else u + ly[j] * ru
            v = ly[0] * rv if j == 0 else v + ly[j] * rv
        return u, v

    def locate(self, px, py, e, hops=0):
        """(status, e, xi, eta, px, py, hops): the location of the target (px, py) starting from the
        0-based element e with `hops` passes through (3) behind it.  In a migrating set a processor face
        gives FLIGHT, and self._dest = (k, pos)."""
        xi = eta = 0.0
        while True:
            c = self._c[e]
            self._through.add(e + 1)
            r = _invert(c, px, py)
            if r is None:
                return LOST, e, xi, eta, px, py, hops
            xi, eta = r
            ax, ay = abs(xi), abs(eta)
            if max(ax, ay) <= 1.0 + self._tol[e]:
                return ACTIVE, e, _clamp(xi), _clamp(eta), px, py, hops
            if hops == 4:
                return LOST, e, xi, eta, px, py, hops
            hops += 1
            in_eta = ay - 1.0 > ax - 1.0
            plus = (eta if in_eta else xi) > 0.0
            nb = self._nbr[e][(2 if in_eta else 0) + (1 if plus else 0)]
            if nb >= 0:
                e = nb
            elif nb == WALL:
                if in_eta:
                    eta = 1.0 if plus else -1.0
                else:
                    xi = 1.0 if plus else -1.0
                x, _ = _bilinear(c, xi, eta)
                px, py = x
                self.walls += 1
            else:
                if self.xface is not None:
                    k, pos = self.xface[e][(2 if in_eta else 0) + (1 if plus else 0)]
                    if k >= 0:
                        self._dest = (k, pos)
                        return FLIGHT, e, xi, eta, px, py, hops
                return LEFT, e, xi, eta, px, py, hops

    def _stop(self, m, status, px, py):
        self.status[m], self.x[m], self.y[m] = status, px, py
        self.elem[m] = 0
        self.wx[m] = self.wy[m] = 0.0

    def _heun(self, q, k, x, y, wx, wy, dt, stage, px, py, e, hops):
        """The advance of (x, y, w) in layer k (0-based) from a stage on (float_plan.h: float_heun): stage 0
        locates p* = (px, py) from e, u* = vel, p1, and goes on as stage 1 with no pass behind it; stage 1
        locates p1 = (px, py), w = vel.  Returns (status, e, xi, eta, px, py, us, vs, stage, hops of the
        last location, most hops of a location)."""
        us = vs = 0.0
        most = 0
        if stage == 0:
            st, e, xi, eta, px, py, h = self.locate(px, py, e, hops)
            most = h
            if st == ACTIVE:
                us, vs = self.vel(q, k, e, xi, eta)
                if not (math.isfinite(us) and math.isfinite(vs)):
                    st = LOST
            if st != ACTIVE:
                return st, e, xi, eta, px, py, us, vs, 0, h, most
            px, py = x + (0.5 * dt) * (wx + us), y + (0.5 * dt) * (wy + vs)
            hops = 0
        st, e, xi, eta, px, py, h = self.locate(px, py, e, hops)
        if st == ACTIVE:
            us, vs = self.vel(q, k, e, xi, eta)
            if not (math.isfinite(us) and math.isfinite(vs)):
                st = LOST
        return st, e, xi, eta, px, py, us, vs, 1, h, max(most, h)

    def _finish(self, m, res, k, x, y, wx, wy, dt):
        """Float m after _heun: it moved, it stopped, or it is in flight (its slot LEFT, a record in the outbox)."""
        st, e, xi, eta, px, py, us, vs, stage, h, most = res
        self.hops[m] = max(self.hops[m], most)
        self.walled[m] = self.walled[m] or self.walls > 0
        if st == FLIGHT:
            self.outbox.append(dict(gid=m, layer=k + 1, x=x, y=y, wx=wx, wy=wy, dt=dt, stage=stage, px=px, py=py, hops=h,
                                    k=self._dest[0], pos=self._dest[1]))
            st = LEFT
        if st != ACTIVE:
            self._stop(m, st, px, py)
            return
        self.status[m] = ACTIVE           # (an arrival's slot was LEFT)
        self.x[m], self.y[m], self.wx[m], self.wy[m] = px, py, us, vs
        self.elem[m], self.xi[m], self.eta[m] = e + 1, xi, eta

    def advance(self, q_df, dt=None):
        """One advance of every ACTIVE float by dt (default: the case's dt) on q_df (3, npoin, L).
        Afterwards: hops (M) = the most hops a location of this advance took per float, walled (M) =
        whether a wall moved a target."""
        q = self._q = np.asarray(q_df)
        dt = float(self.dt if dt is None else dt)
        self.hops = np.zeros(self.M, dtype=np.int32)
        self.walled = np.zeros(self.M, dtype=bool)
        for m in range(self.M):
            if self.status[m] != ACTIVE:
                continue
            k, e = int(self.layer[m]) - 1, int(self.elem[m]) - 1
            x, y = float(self.x[m]), float(self.y[m])
            self.walls = 0
            self._through = self.visited[m]
            if self.fresh[m]:
                self.wx[m], self.wy[m] = self.vel(q, k, e, float(self.xi[m]), float(self.eta[m]))
                self.fresh[m] = 0
                if not (math.isfinite(self.wx[m]) and math.isfinite(self.wy[m])):
                    self._stop(m, LOST, x, y)
                    continue
            wx, wy = float(self.wx[m]), float(self.wy[m])
            self._finish(m, self._heun(q, k, x, y, wx, wy, dt, 0, x + dt * wx, y + dt * wy, e, 0), k, x, y, wx, wy, dt)

    def resume(self, q_df, fl, e):
        """The tail of an advance from the flight record fl (a dict as in outbox) in this rank's 0-based
        element e behind the face: float_plan.h's float_resume, into slot fl["gid"]."""
        m, k = fl["gid"], fl["layer"] - 1
        self._q = np.asarray(q_df)
        self.walls = 0
        self._through = self.visited[m]
        self.fresh[m] = 0
        res = self._heun(np.asarray(q_df), k, fl["x"], fl["y"], fl["wx"], fl["wy"], fl["dt"], fl["stage"], fl["px"], fl["py"], e,
                         fl["hops"])
        self._finish(m, res, k, fl["x"], fl["y"], fl["wx"], fl["wy"], fl["dt"])

    def release(self, idx):
        """The floats idx that are ACTIVE here become LEFT, elem 0, w 0 (hnumo_floats_release)."""
        for m in idx:
            if self.status[m] == ACTIVE:
                self.status[m], self.elem[m] = LEFT, 0
                self.wx[m] = self.wy[m] = 0.0
                self.visited[m] = set()

    after_step = advance

    # ---- read-outs
    def get(self) -> dict:
        return {"x": self.x.copy(), "y": self.y.copy(), "u": self.wx.copy(), "v": self.wy.copy(),
                "elem": self.elem.copy(), "status": self.status.copy()}

    def record(self):
        """x, y, u, v, elem and the S sensor rows on the state of the last advance."""
        rec = np.stack([self.x, self.y, self.wx, self.wy, self.elem.astype(np.float64)])
        if self.sensors:
            rec = np.concatenate([rec, self.sense(self._q)])
        self._records.append(rec)

    def series(self, clear: bool = False):
        out = np.zeros((5 + sense_rows(self.sensors), self.M, len(self._records)), order="F")
        for i, r in enumerate(self._records):
            out[:, :, i] = r
        if clear:
            self._records = []
        return out


class DeviceFloats:
    """The same floats in an hnumo.engine.Engine.  begin(every=1) makes the engine advance them by
    the case's dt after every successful step; advance(dt=...) is an explicit advance on the state on
    the device now."""

    needs_host_state = False

    def __init__(self, engine, xy, layer, xgl=None, coord=None, sensors=0):
        self.engine = engine
        case = engine.case
        self.xy, self.layer = np.asfortranarray(xy, dtype=np.float64), layer
        self.id = engine.floats_create(case.arrays["coord"] if coord is None else coord,
                                       _sample.case_xgl(case) if xgl is None else xgl, self.xy, layer)
        self.every = 0
        self.sensors = 0
        if sensors:
            self.set_sensors(sensors)

    def host_floats(self, coriolis=True):
        """The Python mirror seeded as this set was, with its sensors."""
        return HostFloats(self.engine.case, self.xy, self.layer, sensors=self.sensors, coriolis=coriolis)

    def set_sensors(self, mask):
        """The sensor mask (hnumo_floats_sensors): before begin(); SENSE_VORT after the engine's vort_begin."""
        self.engine.floats_sensors(self.id, mask)
        self.sensors = int(mask)

    def sense(self, q_df=None):
        """(S, M): the sensors on the state on the device now; q_df is ignored."""
        return self.engine.floats_sense(self.id)

    def sense_info(self):
        """(S, K): the sensor rows and the element slots of the sensor kernel's arena."""
        return self.engine.floats_sense_info(self.id)

    def set(self, xy, layer):
        self.xy, self.layer = np.asfortranarray(xy, dtype=np.float64), layer
        self.engine.floats_set(self.id, self.xy, layer)

    def begin(self, every: int = 1, record_every: int = 0, capacity: int = 0):
        self.engine.floats_begin(self.id, every, record_every, capacity)
        self.every = every

    def advance(self, q_df=None, dt=None):
        """An explicit advance by dt (default: the case's dt); q_df is ignored."""
        self.engine.floats_advance(self.id, self.engine.case.scalars["dt"] if dt is None else dt)

    def after_step(self, q_df=None):
        """time_loop's hook: the engine has advanced the set itself when begin(every=1) was called."""
        if self.every != 1:
            self.advance()

    def get(self) -> dict:
        return self.engine.floats_get(self.id)

    def plan(self):
        """(elem (M), xi (M), eta (M)): the cached locations, as a DeviceSampler(elem=, xi_eta=) takes them."""
        elem, xe = self.engine.floats_plan(self.id)
        return elem, xe[0].copy(), xe[1].copy()

    def record(self):
        self.engine.floats_record(self.id)

    def series(self, clear: bool = False):
        return self.engine.floats_series(self.id, clear)

    def destroy(self):
        self.engine.floats_destroy(self.id)


def migrate_tables(part):
    """(xface (ne, 4, 2) int32, arrive [per neighbour: 0-based elements]) of a processor-face rank: the side
    of face(7) that the face at position pos of neighbour k's list lies on gets (k, pos), every other side
    (-1, -1); arrive[k][pos] is that element."""
    A, ngl = part.arrays, part.scalars["ngl"]
    face, imapl = np.asarray(A["face"]), np.asarray(A["imapl"])
    ne = _sample.owned_elements(part)
    xface = np.full((ne, 4, 2), -1, dtype=np.int32)
    arrive = []
    for k, nb in enumerate(part.fneighbours):
        els = []
        for pos, f in enumerate(nb.faces):
            f = int(f)
            el = int(face[6, f])
            if face[7, f] != 0 or not 1 <= el <= ne:
                raise ValueError(f"face {f + 1} is not a processor face of an owned element")
            i, j = imapl[0, :, f], imapl[1, :, f]
            on = [(i == 1).all(), (i == ngl).all(), (j == 1).all(), (j == ngl).all()]
            if sum(on) != 1:
                raise ValueError(f"face {f + 1}: its nodes are not one side of element {el}")
            sd = on.index(True)
            if xface[el - 1, sd, 0] >= 0:
                raise ValueError(f"face {f + 1} lies on a side that is listed already")
            xface[el - 1, sd] = (k, pos)
            els.append(el - 1)
        arrive.append(els)
    return xface, arrive


class HostFloatGroup:
    """The numpy mirror of a migrating set on the ranks `parts` (hnumo.facepart.face_partition cases, in rank
    order): one HostFloats per rank, seeded from the same xy, layer; a seed ACTIVE on several ranks stays on
    the lowest.  advance(states, dt) is hnumo_group_floats_advance on the ranks' synced states.  For the
    tests it keeps, per float, crossings = [(advance, stage, hops, from rank, to rank), ...] and
    path = the ranks that held it after each advance; rounds = the rounds the last advance took."""

    def __init__(self, parts, xy, layer, coord_scale=0.0):
        self.parts = list(parts)
        self.ranks = [HostFloats(p, xy, layer, coord_scale=coord_scale) for p in self.parts]
        self.M = self.ranks[0].M
        self.arrive = []
        for p, hf in zip(self.parts, self.ranks):
            hf.xface, arr = migrate_tables(p)
            hf.xface = [[(int(k), int(pos)) for k, pos in row] for row in hf.xface]
            self.arrive.append(arr)
        self.shared = np.sum([hf.status == ACTIVE for hf in self.ranks], axis=0) > 1
        held = np.zeros(self.M, bool)
        for hf in self.ranks:
            on = hf.status == ACTIVE
            hf.release(np.nonzero(on & held)[0])
            held |= on
        self.crossings = [[] for _ in range(self.M)]
        self.path = [[r for r, hf in enumerate(self.ranks) if hf.status[m] == ACTIVE] for m in range(self.M)]
        self.nadvance = self.rounds = self.max_rounds = 0
        self.in_flight_after = 0

    def neighbour_index(self, r, rank):
        return [nb.rank for nb in self.parts[r].fneighbours].index(rank)

    def advance(self, states, dt=None):
        for hf, q in zip(self.ranks, states):
            hf.outbox = []
            hf.advance(q, dt)
        hops = [hf.hops.copy() for hf in self.ranks]
        walled = [hf.walled.copy() for hf in self.ranks]
        self.rounds = 0
        for rnd in range(MAXROUNDS + 1):
            boxes = [hf.outbox for hf in self.ranks]
            if not any(boxes):
                break
            if rnd == MAXROUNDS:
                for hf, box in zip(self.ranks, boxes):      # (cannot happen) still in flight: LOST where it left
                    for fl in box:
                        hf.status[fl["gid"]] = LOST
                self.in_flight_after += sum(len(b) for b in boxes)
                break
            self.rounds = rnd + 1
            for hf in self.ranks:
                hf.outbox = []
            for r, hf in enumerate(self.ranks):
                for k, nb in enumerate(self.parts[r].fneighbours):
                    me = self.neighbour_index(nb.rank, r)
                    for fl in sorted(boxes[nb.rank], key=lambda f: f["gid"]):
                        if fl["k"] != me:
                            continue
                        self.crossings[fl["gid"]].append((self.nadvance, fl["stage"], fl["hops"], nb.rank, r))
                        hf.resume(states[r], fl, self.arrive[r][k][fl["pos"]])
        for r, hf in enumerate(self.ranks):
            hf.hops, hf.walled = np.maximum(hf.hops, hops[r]), hf.walled | walled[r]
        self.max_rounds = max(self.max_rounds, self.rounds)
        self.nadvance += 1
        for m in range(self.M):
            on = [r for r, hf in enumerate(self.ranks) if hf.status[m] == ACTIVE]
            assert len(on) <= 1, (m, on)
            if on and (not self.path[m] or self.path[m][-1] != on[0]):
                self.path[m].append(on[0])

    def get(self):
        return [hf.get() for hf in self.ranks]

    def record(self):
        for hf in self.ranks:
            hf.record()

    def series(self, clear: bool = False):
        return [hf.series(clear) for hf in self.ranks]


def merge_series(series_per_rank, parts):
    """(5 + S, M, count) from the ranks' series (5 + S, M, count) of one migrating set: for each float and record the
    rank where elem > 0, its element numbered globally (1-based, through parts[r].elems); sensor rows go along.  A float no rank
    holds in a record (it left the domain's ranks, or is LOST) is taken from the rank that held it last, from
    rank 0 if none ever did."""
    sers = [np.asarray(s) for s in series_per_rank]
    out = np.array(sers[0], order="F", copy=True)
    _, M, count = out.shape
    last = np.zeros(M, dtype=np.int64)
    for i in range(count):
        held = np.zeros(M, bool)
        for r, (ser, p) in enumerate(zip(sers, parts)):
            on = ser[4, :, i] > 0
            if (on & held).any():
                raise ValueError(f"record {i}: a float has elem > 0 on two ranks")
            held |= on
            last[on] = r
        for r, (ser, p) in enumerate(zip(sers, parts)):
            take = last == r
            glob = np.concatenate([[0], np.asarray(p.elems[:_sample.owned_elements(p)]) + 1]).astype(np.float64)
            out[:, take, i] = ser[:, take, i]
            out[4, take, i] = glob[ser[4, take, i].astype(np.int64)]
    return out


class GroupFloats:
    """A migrating float set on the engines of a local group (processor-face ranks, in rank order): the same
    xy, layer on every engine, hnumo_group_floats_migrate, and then begin / advance / get / series / destroy;
    get() and series() return one entry per rank (merge_series joins the series)."""

    def __init__(self, engines, xy, layer, coord_scale=0.0, migrate=True, sensors=0):
        from .engine import group_floats_migrate
        self.engines = list(engines)
        self.sets = [DeviceFloats(e, xy, layer, sensors=sensors) for e in self.engines]
        self.id = self.sets[0].id
        if any(s.id != self.id for s in self.sets):
            raise ValueError("the set must get the same id on every engine of the group")
        if migrate:
            group_floats_migrate(self.engines, self.id, True, coord_scale)

    def begin(self, every: int = 1, record_every: int = 0, capacity: int = 0):
        for s in self.sets:
            s.begin(every, record_every, capacity)

    def advance(self, dt=None):
        from .engine import group_floats_advance
        group_floats_advance(self.engines, self.id, self.engines[0].case.scalars["dt"] if dt is None else dt)

    def get(self):
        return [s.get() for s in self.sets]

    def series(self, clear: bool = False):
        return [s.series(clear) for s in self.sets]

    def destroy(self):
        for s in self.sets:
            s.destroy()


def seed_grid(case, nx: int, ny: int, margin: float = 0.05):
    """(2, nx*ny) seeds on a regular nx x ny grid inside the bounding box of the owned nodes, `margin`
    of the box away from its sides; point m = i*ny + j is (x_i, y_j)."""
    if nx < 1 or ny < 1 or not 0.0 <= margin < 0.5:
        raise ValueError("seed_grid: nx, ny >= 1 and 0 <= margin < 0.5")
    n = _sample.owned_elements(case) * case.scalars["ngl"] ** 2
    c = np.asarray(case.arrays["coord"])[0:2, :n]
    lo, hi = c.min(axis=1), c.max(axis=1)
    ax = [lo[d] + (hi[d] - lo[d]) * (margin + (1.0 - 2.0 * margin) * (np.arange(k) + 0.5) / k) for d, k in ((0, nx), (1, ny))]
    xy = np.zeros((2, nx * ny), order="F")
    xy[0] = np.repeat(ax[0], ny)
    xy[1] = np.tile(ax[1], nx)
    return xy


def seed_ring(centre, radius: float, n: int, phase: float = 0.0):
    """(2, n) seeds on the circle of `radius` around `centre`, at the angles phase + 2 pi m / n."""
    if n < 1:
        raise ValueError("seed_ring: n >= 1")
    a = phase + 2.0 * math.pi * np.arange(n) / n
    xy = np.zeros((2, n), order="F")
    xy[0] = centre[0] + radius * np.cos(a)
    xy[1] = centre[1] + radius * np.sin(a)
    return xy


def write_trajectories(path, series, layer, status, sensors=0):
    """One .npz: series (5 + S, M, count) = x, y, u, v, elem and the S sensor rows of the mask `sensors` per
    record, layer (M), status (M); the mask is stored when it is not 0."""
    series = np.asarray(series, dtype=np.float64)
    sensors = int(sensors)
    if sensors < 0 or sensors & ~(SENSE_STATE | SENSE_VORT):
        raise ValueError(f"sensors: the mask must be a sum of SENSE_STATE (1) and SENSE_VORT (2), got {sensors}")
    nrows = 5 + sense_rows(sensors)
    if series.ndim != 3 or series.shape[0] != nrows:
        raise ValueError(f"series: shape {series.shape}, expected ({nrows}, M, count)")
    M = series.shape[1]
    layer = np.broadcast_to(np.asarray(layer, dtype=np.int32), (M,))
    status = np.asarray(status, dtype=np.int32).reshape(-1)
    if status.size != M:
        raise ValueError(f"status: {status.size} entries, expected {M}")
    extra = {"sensors": np.int32(sensors)} if sensors else {}
    with open(path, "wb") as f:
        np.savez(f, series=series, layer=layer, status=status, **extra)


def read_trajectories(path, with_sensors: bool = False):
    """(series, layer, status) of a write_trajectories file; with_sensors: and the sensor mask (0: none stored)."""
    with np.load(path) as z:
        out = z["series"], z["layer"], z["status"]
        return (*out, int(z["sensors"]) if "sensors" in z.files else 0) if with_sensors else out
