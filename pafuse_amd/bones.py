"""Bone lengths held constant along a video: the weighted length of every bone and the covariance-weighted projection of
every frame onto those lengths - the host statement, in numpy, of what bone_lengths_kernel and
bone_project_kernel (csrc/kernels.hpp; pafuse_bone_lengths, pafuse_bone_project) compute.

pose [T,N,J,3] fp32 (N the frames of the video), cov [T,N,J,6] fp32 in the order xx, xy, xz, yy, yz, zz (finish_frames'
"cov") or None - an all-zero covariance, bit for bit - floor in metres (fp32, finite and > 0).  Everything below is fp64, one
rounded operation after the other, no fused multiply-add; a sum written  (a + b) + c  is added in that order; results are
rounded once to fp32.

Tables.  parent int [J]: parent[j] is the joint that joint j's BONE hangs on; an entry outside 0 .. j-1 is read as -1, no
bone (so a parent index is always smaller than its child's and no walk can run on).  mirror int [J] or None: the left/right
partner of joint j, or -1.  The children of a joint are listed once per table, ascending.

Per joint (t, n, j):

  s2 = double(floor)*double(floor)
  E = Sigma + s2*I, the EFFECTIVE covariance:  xx = cov0 + s2  yy = cov3 + s2  zz = cov5 + s2   xy = cov1  xz = cov2  yz = cov4
  the covariance is USABLE under the three leading-minor tests of posesmooth.precision (the same function): det finite,
  xx > 0, c22 > 0, det > 0; a NaN anywhere in it makes it unusable
  E*u for a vector u:  row k = (E_k0*u0 + E_k1*u1) + E_k2*u2;      u.g = (u0*g0 + u1*g1) + u2*g2

lengths(pose, cov, parent, mirror, floor) -> (length [T,J] fp32, dev [T,J] fp32, frames [T,J] int32)

  bone j (parent p), frame n:  d = x_j - x_p,  l = sqrt((d0*d0 + d1*d1) + d2*d2),  u = d/l,  v = u.(E_j*u) + u.(E_p*u)
  the frame TAKES PART iff the six pose values are finite, l is finite and > 0, both covariances are usable and v is finite
  and > 0.   w = 1/v:  a frame is trusted as far as its hypotheses agree ALONG the bone.
  S0 = sum w    S1 = sum w*l    S2 = sum (w*l)*l    and a count
  every sum in rootfit.SUM_ORDER over the frames: lane i of 64 adds the terms of frames i, i + 64, ... in ascending order
  from 0.0 (a frame that takes no part feeds 0.0), then v = v + v[lane ^ o] for o = 32 .. 1.
  With mirror: bone j and bone m = mirror[j] (0 <= m < J, m != j, m itself a bone) POOL their frames: every lane runs on from
  the frames of the lower-indexed bone into the frames of the higher, one running sum, then the butterfly - so partners that
  name each other get the same bits.
  L = S1/S0      var = S2/S0 - L*L      dev = sqrt(var > 0 ? var : 0)       frames = the count
  no bone, or a count of 0:  L = dev = NaN, frames = 0.
  dev is the "bone-length standard deviation" of the INPUT, per bone: the known diagnostic.

project(pose, cov, parent, length, iterations, snap, floor) -> (out [T,N,J,3] fp32, code [T,N,J] uint8, resid [T,N,2] fp32)

  Every (t, n) is independent; L_j = double(length[t, j]).
  A joint without a bone (parent -1: a chain top, such as the root) is PINNED: its E is 0 in everything below and it never
  moves.  Every other joint carries its effective covariance.
  Bone j is ACTIVE in the frame iff it has a parent p, L_j is finite and > 0, the six pose values of j and p are finite and
  the covariances of j and p are both usable (a pinned joint's is tested too, although only its zero is used).
  n_j = [bone j active] + the number of active bones among j's children: fixed per frame.

  y = double(pose); then `iterations` (0 .. 64) Jacobi sweeps, each reading the y of its start:
  phase A, per active bone j:  d = y_j - y_p, l, u as above; the bone SKIPS the sweep (a_j = b_j = 0.0) unless l is finite
     and > 0;  g_c = E_j*u  g_p = E_p*u  s = u.g_c + u.g_p; it skips unless s is finite and > 0;
     lam = (l - L_j)/s   a_j = g_c*lam   b_j = g_p*lam        (the exact minimiser of dc' E_c^-1 dc + dp' E_p^-1 dp under the
     constraint linearised at y: the child moves by -a_j, the parent by +b_j)
  phase B, per joint j with n_j > 0 that is not pinned:  D = 0.0 - a_j if bone j is active, else 0.0; D = D + b_k for the active
     children k ascending;  y_j = y_j + D/double(n_j), component by component.

  snap (after the sweeps, every joint reading the y of their end):  per bone  step_c = (y_c - y_p)*(L_c/l_c), or the unscaled
     difference where l_c is not finite or not > 0.  For a joint j whose bone is active: acc = 0.0; c = j; while bone c is
     active: acc = acc + step_c, c = parent[c] - leaf to root; z_j = y_c + acc with c where the walk ended.  Every other joint:
     z_j = y_j.

  out = fp32(z), or fp32(y) without snap, where n_j > 0: code 1.  A joint with n_j = 0 keeps the INPUT's bits: code 0, or
  code 3 where a bone was asked of it - its own bone or one of its children's has a length in the table (finite and > 0) -
  and a pose that is not finite or a covariance that is not usable made that impossible.  No NaN is created.
  resid[t, n] = (before, after): the largest |l - L| over the active bones of the frame (a bone whose l is not finite counts
  +inf), metres; before on double(pose), after on double(out) - THE FP32 VALUES THAT ARE RETURNED.  NaN: no active bone.

This module is test infrastructure and the documentation of the arithmetic.  The product path never calls it.
"""
import numpy as np

from . import posesmooth
from .rootfit import LANES, lane_sum

KEPT, DONE, FAILED = 0, 1, 3
MAX_JOINTS = 256
MAX_ITERATIONS = 64
SYM = posesmooth.SYM


def check_floor(floor, who="bones"):
    """-> floor as fp32; ValueError unless it is a number that is finite and > 0 in fp32"""
    if isinstance(floor, (bool, np.bool_)) or not isinstance(floor, (int, float, np.floating, np.integer)):
        raise ValueError(f"{who}: floor must be a finite number > 0 (metres), got {floor!r}")
    with np.errstate(all="ignore"):
        f = np.float32(floor)
    if not (np.isfinite(f) and f > 0):
        raise ValueError(f"{who}: floor must be finite and > 0 in fp32 (metres), got {floor!r}")
    return f


def table(parent, J, strict=False):
    """parent -> int64 [J] with every entry outside 0 .. j-1 read as -1 (what the kernels do); strict=True: ValueError for an
    entry outside -1 .. j-1 instead (what the Python layers do)"""
    par = np.asarray(parent)
    if par.shape != (J,) or par.dtype.kind not in "iu":
        raise ValueError(f"bones: parent must be an integer table [J] = [{J}], got {par.dtype} {par.shape}")
    par = par.astype(np.int64)
    j = np.arange(J)
    good = (par >= 0) & (par < j)
    if strict and not (good | (par == -1)).all():
        bad = int(np.flatnonzero(~(good | (par == -1)))[0])
        raise ValueError(f"bones: parent[{bad}] = {int(par[bad])} is outside -1 .. {bad - 1}: every parent index must be smaller than its child's")
    return np.where(good, par, -1)


def children(par):
    """-> the child lists of the (read) table, ascending"""
    kids = [[] for _ in range(len(par))]
    for k, p in enumerate(par):
        if p >= 0:
            kids[p].append(k)
    return kids


def _shapes(pose, cov):
    pose = np.asarray(pose, dtype=np.float32)
    if pose.ndim != 4 or pose.shape[-1] != 3 or 0 in pose.shape:
        raise ValueError(f"bones: pose must be [T,N,J,3] with T, N, J >= 1, got {pose.shape}")
    if pose.shape[2] > MAX_JOINTS:
        raise ValueError(f"bones: J = {pose.shape[2]} is more than {MAX_JOINTS}")
    if cov is not None:
        cov = np.asarray(cov, dtype=np.float32)
        if cov.shape != pose.shape[:3] + (6,):
            raise ValueError(f"bones: cov must be [T,N,J,6] = {pose.shape[:3] + (6,)}, got {cov.shape}")
    return pose, cov


def effective(pose, cov, floor):
    """-> (E [T,N,J,6] fp64 the effective covariance Sigma + floor^2*I, usable [T,N,J] bool: posesmooth.precision's tests)"""
    s2 = np.float64(np.float32(floor)) * np.float64(np.float32(floor))
    E = np.zeros(pose.shape[:3] + (6,)) if cov is None else cov.astype(np.float64)
    E[..., [0, 3, 5]] = E[..., [0, 3, 5]] + s2
    _, usable = posesmooth.precision(np.zeros_like(pose), cov, floor)
    return E, usable


def _matvec(E, u):
    return np.stack([(E[..., SYM[k][0]] * u[..., 0] + E[..., SYM[k][1]] * u[..., 1]) + E[..., SYM[k][2]] * u[..., 2] for k in range(3)], axis=-1)


def _dot(u, g):
    return (u[..., 0] * g[..., 0] + u[..., 1] * g[..., 1]) + u[..., 2] * g[..., 2]


def _norm(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _good(v):
    return np.isfinite(v) & (v > 0)


def bone_sums(pose, cov, parent, floor):
    """-> (w, wl, wll [T,N,J] fp64 - 0.0 where the frame takes no part in bone j - and part [T,N,J] bool): the terms of every
    (frame, bone) before any sum"""
    pose, cov = _shapes(pose, cov)
    par = table(parent, pose.shape[2])
    has, pc = par >= 0, np.maximum(par, 0)
    E, usable = effective(pose, cov, floor)
    y = pose.astype(np.float64)
    fin = np.isfinite(pose).all(axis=-1)
    with np.errstate(all="ignore"):
        d = y - y[:, :, pc]
        l = _norm(d)
        u = d / l[..., None]
        v = _dot(u, _matvec(E, u)) + _dot(u, _matvec(E[:, :, pc], u))
        part = has & fin & fin[:, :, pc] & _good(l) & usable & usable[:, :, pc] & _good(v)
        w = 1.0 / v
        wl = w * l
        wll = wl * l
    z = lambda a: np.where(part, a, 0.0)
    return z(w), z(wl), z(wll), part


def _frames_sum(terms, partner):
    """terms [T,N,J] -> [T,J]: per bone the lane-then-butterfly sum over the frames; partner [J]: -1, or the bone whose frames
    are pooled with this one's - the lower-indexed bone's frames first, every lane running on into the higher's"""
    T, N, J = terms.shape
    rounds = -(-N // LANES)
    x = np.zeros((T, J, rounds * LANES))
    x[:, :, :N] = terms.transpose(0, 2, 1)
    out = np.empty((T, J))
    for j in range(J):
        m = int(partner[j])
        out[:, j] = lane_sum(x[:, j] if m < 0 else np.concatenate([x[:, min(j, m)], x[:, max(j, m)]], axis=-1))
    return out


def partners(par, mirror):
    """-> int64 [J]: the bone every bone pools its frames with, or -1"""
    J = len(par)
    out = np.full(J, -1, dtype=np.int64)
    if mirror is None:
        return out
    mir = np.asarray(mirror)
    if mir.shape != (J,) or mir.dtype.kind not in "iu":
        raise ValueError(f"bones: mirror must be an integer table [J] = [{J}] or None, got {mir.dtype} {mir.shape}")
    for j in range(J):
        m = int(mir[j])
        if par[j] >= 0 and 0 <= m < J and m != j and par[m] >= 0:
            out[j] = m
    return out


def lengths(pose, cov, parent, mirror=None, floor=1e-3):
    """-> (length [T,J] fp32, dev [T,J] fp32, frames [T,J] int32): what pafuse_bone_lengths writes."""
    f = check_floor(floor, "bone_lengths")
    pose, cov = _shapes(pose, cov)
    par = table(parent, pose.shape[2])
    pair = partners(par, mirror)
    w, wl, wll, part = bone_sums(pose, cov, par, f)
    S0, S1, S2 = (_frames_sum(a, pair) for a in (w, wl, wll))
    cnt = part.sum(axis=1).astype(np.int64)
    cnt = cnt + np.where(pair >= 0, cnt[:, np.maximum(pair, 0)], 0)
    with np.errstate(all="ignore"):
        L = S1 / S0
        var = S2 / S0 - L * L
        dev = np.sqrt(np.where(var > 0, var, 0.0))
    none = cnt == 0
    L, dev = np.where(none, np.nan, L), np.where(none, np.nan, dev)
    with np.errstate(all="ignore"):
        return L.astype(np.float32), dev.astype(np.float32), cnt.astype(np.int32)


def check_project(iterations, snap, floor):
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"bone_project: iterations must be an integer in 0 .. {MAX_ITERATIONS}, got {iterations!r}")
    if not isinstance(snap, (bool, np.bool_)) and not (isinstance(snap, (int, np.integer)) and int(snap) in (0, 1)):
        raise ValueError(f"bone_project: snap must be a bool (or 0 / 1), got {snap!r}")
    return int(iterations), bool(snap), check_floor(floor, "bone_project")


def _length_table(length, T, J):
    L = np.asarray(length, dtype=np.float32)
    if L.shape != (T, J):
        raise ValueError(f"bone_project: length must be [T,J] = {(T, J)}, got {L.shape}")
    return L


class Frame:
    """What is fixed per (t, n) before the first sweep: the tables, E with the pinned joints' zeroed, the active bones, n_j"""

    def __init__(self, pose, cov, parent, length, floor):
        self.pose, cov = _shapes(pose, cov)
        T, N, J, _ = self.pose.shape
        self.par = table(parent, J)
        self.has, self.pc = self.par >= 0, np.maximum(self.par, 0)
        self.kids = children(self.par)
        self.ranks = []                                                                # per rank r: (the joints with more than r children, their r-th child)
        for r in range(max((len(k) for k in self.kids), default=0)):
            at = np.array([p for p, ks in enumerate(self.kids) if r < len(ks)])
            self.ranks.append((at, np.array([self.kids[p][r] for p in at])))
        self.L32 = _length_table(length, T, J)
        self.L = self.L32.astype(np.float64)[:, None, :]                                # [T,1,J]
        E, self.usable = effective(self.pose, cov, floor)
        E[:, :, ~self.has] = 0.0                                                       # pinned
        self.E, self.Ep = E, E[:, :, self.pc]
        self.fin = np.isfinite(self.pose).all(axis=-1)
        with np.errstate(all="ignore"):
            self.asked = self.has & _good(self.L32)[:, None, :]                         # [T,1,J] -> broadcasts
        self.asked = np.broadcast_to(self.asked, (T, N, J))
        self.active = self.asked & self.fin & self.fin[:, :, self.pc] & self.usable & self.usable[:, :, self.pc]
        self.count = self.active.astype(np.int64)
        self.wanted = self.asked.copy()                                                 # a bone was asked of the joint
        for p, ks in enumerate(self.kids):
            for k in ks:
                self.count[:, :, p] += self.active[:, :, k]
                self.wanted[:, :, p] |= self.asked[:, :, k]

    def bones(self, y):
        """-> (d, l, fine): the difference and length of every bone at y, and where l is finite and > 0"""
        with np.errstate(all="ignore"):
            d = y - y[:, :, self.pc]
            l = _norm(d)
            return d, l, _good(l)

    def phase_a(self, y):
        with np.errstate(all="ignore"):
            d, l, fine = self.bones(y)
            u = d / l[..., None]
            gc, gp = _matvec(self.E, u), _matvec(self.Ep, u)
            s = _dot(u, gc) + _dot(u, gp)
            go = (self.active & fine & _good(s))[..., None]
            lam = ((l - self.L) / s)[..., None]
            return np.where(go, gc * lam, 0.0), np.where(go, gp * lam, 0.0)

    def sweep(self, y):
        a, b = self.phase_a(y)
        D = np.where(self.active[..., None], 0.0 - a, 0.0)
        for at, k in self.ranks:                                                        # the r-th child of the joints `at` that have one
            D[:, :, at] = D[:, :, at] + np.where(self.active[:, :, k][..., None], b[:, :, k], 0.0)
        move = (self.count > 0) & self.has
        with np.errstate(all="ignore"):
            return np.where(move[..., None], y + D / self.count.astype(np.float64)[..., None], y)

    def snap(self, y):
        T, N, J, _ = y.shape
        with np.errstate(all="ignore"):
            d, l, fine = self.bones(y)
            step = np.where(fine[..., None], d * (self.L / l)[..., None], d)
        acc = np.zeros_like(y)
        cur = np.broadcast_to(np.arange(J), (T, N, J)).copy()
        for _ in range(J):
            on = np.take_along_axis(self.active, cur, axis=2)
            if not on.any():
                break
            acc = np.where(on[..., None], acc + np.take_along_axis(step, cur[..., None], axis=2), acc)
            cur = np.where(on, self.pc[cur], cur)
        return np.where(self.active[..., None], np.take_along_axis(y, cur[..., None], axis=2) + acc, y)

    def resid(self, y):
        """the largest |l - L| over the active bones of every frame, NaN where there is none -> [T,N] fp64"""
        with np.errstate(all="ignore"):
            _, l, _ = self.bones(y)
            e = np.where(np.isfinite(l), np.abs(l - self.L), np.inf)
        e = np.where(self.active, e, -np.inf).max(axis=-1)
        return np.where(self.active.any(axis=-1), e, np.nan)


def project_f64(pose, cov, parent, length, iterations, snap, floor):
    """-> (value [T,N,J,3] fp64 before its rounding, the Frame)"""
    fr = Frame(pose, cov, parent, length, floor)
    y = fr.pose.astype(np.float64)
    for _ in range(iterations):
        y = fr.sweep(y)
    return (fr.snap(y) if snap else y), fr


def project(pose, cov, parent, length, iterations=16, snap=True, floor=1e-3):
    """-> (out [T,N,J,3] fp32, code [T,N,J] uint8, resid [T,N,2] fp32): what pafuse_bone_project writes."""
    it, snap, f = check_project(iterations, snap, floor)
    z, fr = project_f64(pose, cov, parent, length, it, snap, f)
    touched = fr.count > 0
    with np.errstate(all="ignore"):
        out = np.where(touched[..., None], z.astype(np.float32), fr.pose)             # else the bits of the input
    code = np.where(touched, DONE, np.where(fr.wanted, FAILED, KEPT)).astype(np.uint8)
    with np.errstate(all="ignore"):
        resid = np.stack([fr.resid(fr.pose.astype(np.float64)), fr.resid(out.astype(np.float64))], axis=-1).astype(np.float32)
    return out, code, resid
